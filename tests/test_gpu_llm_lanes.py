"""Lanes: up to eight prompts decoded in lock step (kjarni_hip_decoder_generate_batch and its hooks).

One lane step against the references, ragged (prompts of different lengths, a lane that fills its cache, frozen lanes);
production widths on the multi-row weight-streaming kernel, with the route counter; batched greedy against the oracle and
against generate() prompt by prompt (lane reuse, per-prompt limits, stop ids, the lane capacity, callbacks); logits
processors in lanes; errors.  Float bar: the decoder's, max |gpu - ref| <= 1e-4 * max(1, max |ref|)."""
import numpy as np
import pytest

from oracle import llm_oracle as L
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import llm_ref64, synth
from tests.gpt2_ref64 import Gpt2Ref64

pytestmark = pytest.mark.gpu
TOL = 1e-4
STEPS = 6


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _within(got, ref, what):
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), _bar(ref)
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


class _LlamaRef:
    """Per lane: the oracle's hidden / logits rows and the float64 K / V cache."""

    def __init__(self, t, cfg):
        self.orc, self.r64, self.vocab = L.LlmOracle(t, cfg), llm_ref64.Ref64(t, cfg), cfg["vocab_size"]
        self.first_id = 4

    def new(self):
        return [self.orc.new_cache(), self.r64.new_cache()]

    def forward(self, ids, state):
        self.r64.forward(ids, state[1])
        h = self.orc.forward(ids, state[0])[0][-1]
        return h, self.orc.logits(h)

    def cache(self, state):
        return state[1]


class _Gpt2Ref:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = Gpt2Ref64(t, cfg), cfg["vocab_size"], 0

    def new(self):
        return self.ref.new_cache()

    def forward(self, ids, state):
        h, lg = self.ref.forward(list(ids), state)
        return h[-1], lg

    def cache(self, state):
        return state


def _check_caches(dec, ref, states, lanes, what):
    for l in lanes:
        cache = ref.cache(states[l])
        assert dec.lane_cache_len(l) == cache[0][0].shape[0], f"{what}: lane {l} length"
        got = [dec.lane_kv_rows(l, i) for i in range(len(cache))]
        for (layer, name), (err, bar) in llm_ref64.cache_errors(got, cache).items():
            assert err <= bar, f"{what}: lane {l} layer {layer} {name}: {err:.3e} > {bar:.3e}"


def _run_lane_steps(dec, ref, lens, seed, lane_context=0, freeze=()):
    """Prefill len(lens) lanes, then STEPS lock-step steps; lanes in `freeze` stop after 3 steps, a lane whose cache is
    full stops there (its position is then the capacity: nothing may be written for it)."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    dec.lanes_begin(n, lane_context)
    cap = dec.lane_capacity()
    states = [ref.new() for _ in range(n)]
    for l, m in enumerate(lens):
        ids = rng.integers(ref.first_id, ref.vocab, m).tolist()
        ref.forward(ids, states[l])
        dec.lane_prefill(l, ids)
    _check_caches(dec, ref, states, range(n), "after prefill")
    frozen_rows = {}
    for step in range(STEPS):
        live = [int(dec.lane_cache_len(l) < cap and not (l in freeze and step >= 3)) for l in range(n)]
        for l in range(n):
            if not live[l] and l not in frozen_rows:
                frozen_rows[l] = (dec.lane_cache_len(l), [dec.lane_kv_rows(l, i) for i in range(dec.layers)])
        ids = rng.integers(ref.first_id, ref.vocab, n).tolist()
        hidden, logits = dec.lanes_step(ids, live)
        for l in range(n):
            if live[l]:
                h_ref, l_ref = ref.forward([ids[l]], states[l])
                _within(hidden[l], h_ref, f"step {step} lane {l} hidden")
                _within(logits[l], l_ref, f"step {step} lane {l} logits")
    for l, (length, rows) in frozen_rows.items():  # a frozen lane: same length, the same rows bit for bit
        assert dec.lane_cache_len(l) == length, f"frozen lane {l} grew"
        for i in range(dec.layers):
            k, v = dec.lane_kv_rows(l, i)
            assert np.array_equal(k, rows[i][0]) and np.array_equal(v, rows[i][1]), f"frozen lane {l} layer {i} rewritten"
    _check_caches(dec, ref, states, range(n), "after the steps")
    return frozen_rows


def _llama(tmp_path, base, seed, **kw):
    import kjarni_amd
    d = str(tmp_path / f"{base['model_type']}-{seed}")
    weights = kw.pop("weights", "auto")
    cfg, t = synth.llm_model(d, base, seed=seed, **kw)
    return kjarni_amd.HipDecoder(d, weights=weights), t, cfg


def _lens(cap):
    return [1, 2, 7, 8, 23, 24, 40, cap - 2]   # the last lane has room for two steps, then its position is the capacity


@pytest.mark.parametrize("base", [synth.LLAMA_TEST, synth.QWEN_TEST], ids=["llama-gqa-rope-scaling", "qwen2-bias-mqa-untied"])
def test_lane_steps_against_float64_ragged(tmp_path, base):
    dec, t, cfg = _llama(tmp_path, base, 3)
    ref = _LlamaRef(t, cfg)
    cap = cfg["max_position_embeddings"]
    frozen = _run_lane_steps(dec, ref, _lens(cap), seed=0)
    assert 7 in frozen and frozen[7][0] == cap                       # the full lane stopped at its capacity
    frozen = _run_lane_steps(dec, ref, _lens(cap), seed=1, freeze=(2, 5))
    assert {2, 5, 7} <= set(frozen)
    for lens in ([40, 1], [7, 24, 2], [8, 23, 1, 40, 2]):              # 2, 3 and 5 lanes
        _run_lane_steps(dec, ref, lens, seed=len(lens))
    frozen = _run_lane_steps(dec, ref, [1, 2, 7, 8, 23, 24, 40, 62], seed=5, lane_context=64)  # lanes shorter than the context
    assert dec.lane_capacity() == 64 and frozen[7][0] == 64


def test_lane_steps_gpt2_against_float64_ragged(tmp_path):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(**G.SMALL)
    d = str(tmp_path / "gpt2")
    _, t = G.gpt2_model(d, cfg, seed=1)
    dec, ref = HipDecoder(d, 0), _Gpt2Ref(t, cfg)
    cap = cfg["n_ctx"]
    frozen = _run_lane_steps(dec, ref, _lens(cap), seed=0)
    assert frozen[7][0] == cap
    _run_lane_steps(dec, ref, _lens(cap), seed=1, freeze=(0, 6))
    for lens in ([40, 1], [7, 24, 2], [8, 23, 1, 40, 2]):
        _run_lane_steps(dec, ref, lens, seed=len(lens))


# ---- production widths: the multi-row weight-streaming kernel, by the route counter ------------------------------------------

def _steps_with_counter(dec, ref, lanes, seed, steps=2):
    rng = np.random.default_rng(seed)
    dec.lanes_begin(lanes)
    states = [ref.new() for _ in range(lanes)]
    for l, m in enumerate([3, 9, 1, 30, 2, 8, 17, 5][:lanes]):   # 8-row passes and (30 rows) the matrix-core route
        ids = rng.integers(ref.first_id, ref.vocab, m).tolist()
        ref.forward(ids, states[l])
        dec.lane_prefill(l, ids)
    s0, f0 = dec.lane_gemv_calls()
    for step in range(steps):
        ids = rng.integers(ref.first_id, ref.vocab, lanes).tolist()
        hidden, logits = dec.lanes_step(ids)
        for l in range(lanes):
            h_ref, l_ref = ref.forward([ids[l]], states[l])
            _within(hidden[l], h_ref, f"step {step} lane {l} hidden")
            _within(logits[l], l_ref, f"step {step} lane {l} logits")
    s1, f1 = dec.lane_gemv_calls()
    return (s1 - s0) // steps, (f1 - f0) // steps


FULL_WIDTH = dict(synth.LLAMA_TEST, hidden_size=2048, num_hidden_layers=1, num_attention_heads=32, num_key_value_heads=8,
                  intermediate_size=8192, vocab_size=20011, max_position_embeddings=512, head_dim=64)  # test_full_width_decode_step's
FULL_WIDTH["rope_scaling"] = dict(FULL_WIDTH["rope_scaling"], original_max_position_embeddings=128)


@pytest.mark.parametrize("store_bf16", [True, False], ids=["bf16-weights", "f32-weights"])
def test_llama_1b_widths_take_the_streaming_kernel(tmp_path, store_bf16):
    """Hidden 2048, inner 8192 (two and four K-slices of the down projection), 32 / 8 heads of 64, a looping vocabulary head:
    Q|K|V, o-proj, gate/up, down and the head -- five projections per step -- all on the multi-row weight-streaming kernel."""
    dec, t, cfg = _llama(tmp_path, FULL_WIDTH, 9, bf16_values=True, store_bf16=store_bf16)
    ref = _LlamaRef(t, cfg)
    for lanes in (8, 5):
        assert _steps_with_counter(dec, ref, lanes, seed=lanes) == (5, 0)


@pytest.mark.parametrize("store_bf16", [True, False], ids=["bf16-weights", "f32-weights"])
def test_gpt2_small_widths_take_the_streaming_kernel(tmp_path, store_bf16):
    """768 / 3072 (K-slices of 1 024: one for c_attn, attn.c_proj, c_fc and the head, three for mlp.c_proj), LayerNorm, biases."""
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(n_embd=768, n_layer=1, n_head=12, n_ctx=128, vocab_size=1003)
    d = str(tmp_path / "gpt2-small")
    _, t = G.gpt2_model(d, cfg, seed=2, store_bf16=store_bf16, std=0.02)
    dec, ref = HipDecoder(d, 0), _Gpt2Ref(t, cfg)
    assert dec.bf16 == store_bf16
    for lanes in (8, 5):
        assert _steps_with_counter(dec, ref, lanes, seed=lanes) == (5, 0)


def test_rows_shorter_than_512_fall_back(tmp_path):
    """Hidden 256, inner 512: every projection that reads 256-wide rows takes the one-wave-per-column kernel (Q|K|V, o-proj,
    gate/up, the head), the down projection (512-wide rows) the streaming kernel -- same bar."""
    base = dict(synth.LLAMA_TEST, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512, head_dim=64,
                num_hidden_layers=1)
    dec, t, cfg = _llama(tmp_path, base, 9)
    assert _steps_with_counter(dec, _LlamaRef(t, cfg), 8, seed=1) == (1, 4)


# ---- batched greedy == single-stream greedy == the oracle ----------------------------------------------------------------------

VARIED = [0, 1, 5, 32, 2, 7, 32, 3, 16, 1, 9]


@pytest.mark.parametrize("name", sorted(LC.GREEDY_MODELS))
def test_batched_greedy_equals_single_stream(tmp_path, name):
    base, seed = LC.GREEDY_MODELS[name]
    dec, t, cfg = _llama(tmp_path, base, seed)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(seed, cfg["vocab_size"])
    assert len(ps) == LC.N_PROMPTS and all(1 <= len(p) <= 39 for p in ps)
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP, f"precondition: the oracle's two best logits come within {gap:.2e}"
    single = [dec.generate(p, LC.MAX_NEW) for p in ps]
    assert single == exp
    for lanes in (1, 3, 8):                                            # 11 prompts: every lane count reuses lanes
        assert dec.generate_batch(ps, LC.MAX_NEW, lanes=lanes) == exp, lanes
    assert dec.generate_batch(ps, LC.MAX_NEW) == dec.generate_batch(ps, LC.MAX_NEW) == exp   # lanes = 0 -> 8, twice
    assert [dec.generate(p, LC.MAX_NEW) for p in ps] == single          # a plain generate() after batches
    # per-prompt limits
    exp_v, gap = LC.oracle_runs(orc, ps, VARIED)
    assert gap >= LC.GAP
    for lanes in (1, 3, 8):
        assert dec.generate_batch(ps, VARIED, lanes=lanes) == exp_v == [e[:m] for e, m in zip(exp, VARIED)], lanes
    # the lane capacity: a 45-token prompt in 48-row lanes ends after 3 tokens, the others run on to their own limits
    ps48 = list(ps)
    ps48[3] = np.random.default_rng(seed + 100).integers(4, cfg["vocab_size"], 45).tolist()
    exp48, gap = LC.oracle_runs(orc, ps48, LC.MAX_NEW, context_limit=48)
    assert gap >= LC.GAP
    assert len(exp48[3]) == 3 and max(len(e) for e in exp48) == LC.MAX_NEW
    for lanes in (3, 8):
        assert dec.generate_batch(ps48, LC.MAX_NEW, lanes=lanes, lane_context=48) == exp48, lanes


def test_stop_ids_end_lanes_at_different_steps(tmp_path):
    dec, t, cfg = _llama(tmp_path, LC.EOS_BASE, LC.EOS_SEED)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(LC.EOS_SEED, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    ends = LC.stop_steps(orc, ps, LC.MAX_NEW)
    assert len(ends) >= 2 and len(set(ends.values())) >= 2, ends       # precondition: two prompts stop, at different steps
    for lanes in (1, 3, 8):
        got = dec.generate_batch(ps, LC.MAX_NEW, lanes=lanes)
        assert got == exp == [dec.generate(p, LC.MAX_NEW) for p in ps], lanes
        assert all(tok not in cfg["eos_token_id"] for ids in got for tok in ids)


def test_callbacks_step_major_and_cancel_one_prompt(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    ps = LC.prompts(seed, cfg["vocab_size"])[:5]
    full = dec.generate_batch(ps, 12, lanes=8)
    seen = []
    assert dec.generate_batch(ps, 12, lanes=8, on_token=lambda i, tok: seen.append((i, tok))) == full
    # five prompts in five lanes: the first tokens as the lanes are filled, then step by step, lane order within a step
    assert seen == [(i, full[i][s]) for s in range(12) for i in range(5)]
    seen = []

    def stop_two(i, tok):
        seen.append((i, tok))
        return not (i == 2 and sum(1 for j, _ in seen if j == 2) == 4)
    got = dec.generate_batch(ps, 12, lanes=8, on_token=stop_two)
    assert got[2] == full[2][:4] and [g for i, g in enumerate(got) if i != 2] == [f for i, f in enumerate(full) if i != 2]
    assert [tok for i, tok in seen if i == 2] == full[2][:4]
    # with fewer lanes than prompts the order is still per prompt the generation order
    seen = []
    assert dec.generate_batch(ps, 12, lanes=2, on_token=lambda i, tok: seen.append((i, tok))) == full
    for i in range(5):
        assert [tok for j, tok in seen if j == i] == full[i]


# ---- logits processors in lanes ------------------------------------------------------------------------------------------------

def test_processors_in_lanes_equal_prompt_by_prompt(tmp_path):
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, LC.PROCESSOR_SEED)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(LC.PROCESSOR_SEED, cfg["vocab_size"])
    kw = dict(repetition_penalty=1.3, no_repeat_ngram=2)
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW, **kw)
    assert gap >= LC.GAP, f"precondition: {gap:.2e}"                 # so the tie rule of test_gpu_llm._check never fires
    single = [dec.generate(p, LC.MAX_NEW, **kw) for p in ps]
    assert single == exp
    for lanes in (1, 3, 8):
        assert dec.generate_batch(ps, LC.MAX_NEW, lanes=lanes, **kw) == single, lanes
    assert dec.generate_batch(ps, VARIED, lanes=3, **kw) == [s[:m] for s, m in zip(single, VARIED)]


# ---- errors --------------------------------------------------------------------------------------------------------------------

def test_errors(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    assert dec.generate_batch([], 5) == []
    with pytest.raises(KjarniException, match="prompt 1"):
        dec.generate_batch([[5, 6], [], [7]], 5)                        # an empty prompt, named by its index
    seen = []
    with pytest.raises(KjarniException, match="prompt 2") as e:
        dec.generate_batch([[5, 6], [7], list(range(4, 4 + 49))], 5, lane_context=48, on_token=lambda i, tok: seen.append(tok))
    assert e.value.code == E.INVALID_CONFIG and seen == []              # before any GPU work: nothing was generated
    with pytest.raises(KjarniException) as e:
        dec.generate_batch([[5, 6]], 5, lanes=9)
    assert e.value.code == E.INVALID_CONFIG
    assert dec.generate_batch([[5, 6]], 3, lanes=8) == [dec.generate([5, 6], 3)]
