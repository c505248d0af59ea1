"""Prompt-lookup speculative decoding on the GPU (kjarni_hip_decoder_generate_lookup and its hooks).

The draft kernel against the normative rule; one verify step against float64 (every logits row, the picks, the cache after
rejected rows were overwritten); production widths on the multi-row weight-streaming kernel, by the route counter; the
loop end to end against the oracle's greedy ids (stops, limits, callbacks, the end of the cache); GPT-2 and GGUF stacks; the
Generator.  Float bar: the decoder's, max |gpu - ref| <= 1e-4 * max(1, max |ref|).  Token comparisons carry the
precondition that the reference's two best logits are >= LC.GAP apart at every step, asserted here.

The case builders (`_verify_cases`, `_trace64`, `LK.simulate`) touch no GPU, so every precondition can be evaluated anywhere."""
import os

import numpy as np
import pytest

from oracle import llm_oracle as L
from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import llm_ref64, synth
from tests import lookup_cases as LK
from tests.gpt2_ref64 import Gpt2Ref64

pytestmark = pytest.mark.gpu
TOL = 1e-4
VERIFY_LENS = (1, 7, 8, 23, 24, 40)
# (n_draft, rows, j): the draft is the reference's continuation, with position j replaced by another id when j is not None
SCENARIOS = [(7, 8, None), (7, 8, 0), (7, 8, 2), (7, 8, 6),
             (3, 4, None), (3, 8, None), (3, 4, 2), (3, 8, 0),
             (1, 2, None), (1, 8, None), (1, 2, 0)]
AHEAD = 11   # reference tokens per prompt: the first pick, 7 drafted, the correction, and the two of the step after


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _within(got, ref, what):
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), _bar(ref)
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


# ---- float64 references with every row's logits ------------------------------------------------------------------------------

class _Llama64:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = llm_ref64.Ref64(t, cfg), cfg["vocab_size"], 4
        tied = cfg.get("tie_word_embeddings", cfg["model_type"] == "llama") or "lm_head.weight" not in t
        self.head = self.ref.t["model.embed_tokens.weight" if tied else "lm_head.weight"]

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        """Appends ids; the logits of every new row [len(ids), vocab]."""
        h = self.ref.forward(list(ids), cache)
        return self.ref.rms_norm(h, self.ref.t["model.norm.weight"]) @ self.head.T


class _Gpt264:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = Gpt2Ref64(t, cfg), cfg["vocab_size"], 0

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        hidden, _ = self.ref.forward(list(ids), cache)
        return hidden @ self.ref.t["wte.weight"].T


def _last_max(row):
    return int(len(row) - 1 - np.argmax(row[::-1]))


def _trace64(ref, prompt, n):
    """n greedy tokens of the float64 reference (last maximum wins) and the smallest gap between its two best logits."""
    cache = ref.new()
    row = ref.logits(prompt, cache)[-1]
    out, gap = [], float("inf")
    for _ in range(n):
        top = np.partition(row, -2)[-2:]
        gap = min(gap, float(top[1] - top[0]))
        out.append(_last_max(row))
        row = ref.logits([out[-1]], cache)[-1]
    return out, gap


def _verify_cases(ref, seed):
    """[(prompt, continuation)] for VERIFY_LENS, with the precondition asserted: AHEAD tokens, two best logits >= GAP apart."""
    rng = np.random.default_rng(seed)
    cases = []
    for n in VERIFY_LENS:
        prompt = rng.integers(ref.first_id, ref.vocab, n).tolist()
        cont, gap = _trace64(ref, prompt, AHEAD)
        assert gap >= LC.GAP, f"precondition: prompt of {n}: the reference's two best logits come within {gap:.2e}"
        cases.append((prompt, cont))
    return cases


def _check_cache(dec, ref_cache, what):
    assert dec.cache_len() == ref_cache[0][0].shape[0], what
    got = [dec.kv_rows(i) for i in range(len(ref_cache))]
    for (layer, name), (err, bar) in llm_ref64.cache_errors(got, ref_cache).items():
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e}"


def _run_verify_scenarios(dec, ref, cases):
    for prompt, cont in cases:
        for n_draft, rows, j in SCENARIOS:
            what = f"prompt {len(prompt)} draft {n_draft} rows {rows} wrong at {j}"
            draft = list(cont[1:1 + n_draft])
            if j is not None:
                draft[j] = ref.first_id + (draft[j] - ref.first_id + 1) % (ref.vocab - ref.first_id)   # a different id
            want_a = n_draft if j is None else j
            dec.reset()
            dec.forward(prompt, fetch=False)
            cache = ref.new()
            ref.logits(prompt, cache)
            before = dec.cache_len()
            picks, a, logits = dec.verify_step(cont[0], draft, rows)
            assert a == want_a and picks == cont[1:a + 2], what
            assert dec.cache_len() == before + a + 1, what
            # every row: the model's output after cont[0], draft[0..i) -- the draft as given, rejected positions included
            probe = list(cache)
            want = ref.logits([cont[0]] + draft, probe)
            assert logits.shape == want.shape
            for i in range(n_draft + 1):
                _within(logits[i], want[i], f"{what}: logits row {i}")
            # one more step: it overwrites the rows of the rejected and pad positions; then every cache row is checked
            picks2, a2, logits2 = dec.verify_step(cont[a + 1], [cont[a + 2]], 2)
            ref.logits([cont[0]] + draft[:a], cache)
            want2 = ref.logits([cont[a + 1], cont[a + 2]], cache)
            assert a2 == 1 and picks2 == cont[a + 2:a + 4], what
            for i in range(2):
                _within(logits2[i], want2[i], f"{what}: next step row {i}")
            _check_cache(dec, cache, what)


def _llama(tmp_path, base, seed, **kw):
    import kjarni_amd
    d = str(tmp_path / f"{base['model_type']}-{seed}")
    weights, ctx = kw.pop("weights", "auto"), kw.pop("max_context", 0)
    cfg, t = synth.llm_model(d, base, seed=seed, **kw)
    return kjarni_amd.HipDecoder(d, weights=weights, max_context=ctx), t, cfg


# ---- 1. the draft kernel ---------------------------------------------------------------------------------------------------

def test_draft_kernel_equals_the_rule():
    from kjarni_amd import ops
    for T, (D, hi, lo) in LK.histories():
        assert ops.lookup_draft(T, D, hi, lo) == LK.lookup_draft(T, hi, lo, D), (T, D, hi, lo)
    for _, T, (D, hi, lo) in LK.EDGE_CASES:
        assert ops.lookup_draft(T, D, hi, lo) == LK.lookup_draft(T, hi, lo, D), T
    # the workgroup loop and the reduction over it: more positions than threads, many equal keys
    rng = np.random.default_rng(5)
    for n in (4097, 20000):
        T = rng.integers(0, 3, n).tolist()
        for D, hi, lo in ((7, 3, 1), (7, 4, 4), (2, 1, 1), (5, 4, 2)):
            assert ops.lookup_draft(T, D, hi, lo) == LK.lookup_draft(T, hi, lo, D), (n, D, hi, lo)


# ---- 2. one verify step against float64 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("base", [synth.LLAMA_TEST, synth.QWEN_TEST], ids=["llama-gqa-rope-scaling", "qwen2-bias-mqa-untied"])
def test_verify_step_against_float64(tmp_path, base):
    dec, t, cfg = _llama(tmp_path, base, 3)
    ref = _Llama64(t, cfg)
    _run_verify_scenarios(dec, ref, _verify_cases(ref, 0 if base is synth.LLAMA_TEST else 1))   # (prompt seeds that clear the gap)


def test_verify_step_gpt2_against_float64(tmp_path):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(**G.SMALL)
    d = str(tmp_path / "gpt2")
    _, t = G.gpt2_model(d, cfg, seed=1)
    ref = _Gpt264(t, cfg)
    _run_verify_scenarios(HipDecoder(d, 0), ref, _verify_cases(ref, 0))


# ---- 3. routes: production widths take the multi-row weight-streaming kernel ------------------------------------------------

FULL_WIDTH = dict(synth.LLAMA_TEST, hidden_size=2048, num_hidden_layers=1, num_attention_heads=32, num_key_value_heads=8,
                  intermediate_size=8192, vocab_size=20011, max_position_embeddings=512, head_dim=64)
FULL_WIDTH["rope_scaling"] = dict(FULL_WIDTH["rope_scaling"], original_max_position_embeddings=128)


def _route_steps(dec, ref, seed):
    """A verify step of 8 rows and one of 5 on a 9-token prompt, every logits row within the bar: the counter deltas."""
    rng = np.random.default_rng(seed)
    prompt = rng.integers(ref.first_id, ref.vocab, 9).tolist()
    dec.reset()
    dec.forward(prompt, fetch=False)
    cache = ref.new()
    ref.logits(prompt, cache)
    deltas = []
    for rows in (8, 5):
        ids = rng.integers(ref.first_id, ref.vocab, rows).tolist()
        s0, f0 = dec.verify_gemv_calls()
        picks, a, logits = dec.verify_step(ids[0], ids[1:], rows)
        s1, f1 = dec.verify_gemv_calls()
        deltas.append((s1 - s0, f1 - f0))
        want = ref.logits(ids, list(cache))
        for i in range(rows):
            _within(logits[i], want[i], f"{rows} rows: logits row {i}")
        assert picks[:a] == ids[1:1 + a] and len(picks) == a + 1
        ref.logits(ids[:a + 1], cache)
    _check_cache(dec, cache, "after both steps")
    return deltas


@pytest.mark.parametrize("store_bf16", [True, False], ids=["bf16-weights", "f32-weights"])
def test_llama_1b_widths_take_the_streaming_kernel(tmp_path, store_bf16):
    dec, t, cfg = _llama(tmp_path, FULL_WIDTH, 9, bf16_values=True, store_bf16=store_bf16)
    assert _route_steps(dec, _Llama64(t, cfg), 1) == [(5, 0), (5, 0)]    # Q|K|V, o-proj, gate/up, down, the head


@pytest.mark.parametrize("store_bf16", [True, False], ids=["bf16-weights", "f32-weights"])
def test_gpt2_small_widths_take_the_streaming_kernel(tmp_path, store_bf16):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(n_embd=768, n_layer=1, n_head=12, n_ctx=128, vocab_size=1003)
    d = str(tmp_path / "gpt2-small")
    _, t = G.gpt2_model(d, cfg, seed=2, store_bf16=store_bf16, std=0.02)
    dec = HipDecoder(d, 0)
    assert dec.bf16 == store_bf16
    assert _route_steps(dec, _Gpt264(t, cfg), 2) == [(5, 0), (5, 0)]


def test_rows_shorter_than_512_fall_back(tmp_path):
    base = dict(synth.LLAMA_TEST, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512, head_dim=64,
                num_hidden_layers=1)
    dec, t, cfg = _llama(tmp_path, base, 9)
    assert _route_steps(dec, _Llama64(t, cfg), 3) == [(1, 4), (1, 4)]    # only the down projection reads 512-wide rows


# ---- 4. end to end == the oracle ---------------------------------------------------------------------------------------------

def _greedy_case(name):
    base, seed = LC.GREEDY_MODELS[name]
    return base, seed


def _check_stats(st, out, sim, max_new):
    assert st["drafted_tokens"] >= st["accepted_tokens"]
    assert st["accepted_tokens"] + st["verify_steps"] + st["single_row_steps"] >= len(out) - 1
    assert st["single_row_steps"] == 0
    # the steps the host consumed are the simulated ones, all but the last with the simulated acceptance (the last one's may
    # reach past the end of the output); a run that ends on a stop id may have met it as the first pick of one more step
    extra = st["verify_steps"] - len(sim)
    assert extra == 0 or (extra == 1 and len(out) < max_new)
    body = sum(a for _, a in sim[:-1])
    if extra == 0:
        assert st["drafted_tokens"] == sum(m for m, _ in sim)
        assert body + (sim[-1][1] if sim else 0) <= st["accepted_tokens"] <= body + (sim[-1][0] if sim else 0)
    else:
        assert st["drafted_tokens"] >= sum(m for m, _ in sim) and st["accepted_tokens"] >= body + (sim[-1][1] if sim else 0)


@pytest.mark.parametrize("name", sorted(LC.GREEDY_MODELS))
def test_lookup_equals_the_oracle(tmp_path, name):
    base, seed = _greedy_case(name)
    dec, t, cfg = _llama(tmp_path, base, seed)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(seed, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP, f"precondition: the oracle's two best logits come within {gap:.2e}"
    sims = {D: [LK.simulate(p, e, (D, 3, 1)) for p, e in zip(ps, exp)] for D in (1, 3, 7)}
    accepted = [a for sim in sims[7] for _, a in sim]
    drafted = [m for sim in sims[7] for m, _ in sim]
    if name == "qwen-7":   # coverage: every acceptance count below a full draft, partial acceptances, full misses
        assert len(accepted) == 224 and set(accepted) == set(range(7))
        assert sum(1 for m, a in zip(drafted, accepted) if 0 < a < m) == 24 and sum(1 for m, a in zip(drafted, accepted) if m and not a) == 15
    else:                  # coverage: full 7-token drafts are accepted (33 of 66 steps; llama-7: 31 of 69)
        assert sum(1 for m, a in zip(drafted, accepted) if m == 7 and a == 7) >= 31
    for D in (1, 3, 7):
        for p, e, sim in zip(ps, exp, sims[D]):
            got, st = dec.generate_lookup(p, LC.MAX_NEW, draft_tokens=D)
            assert got == e, (D, len(p))
            _check_stats(st, got, sim, LC.MAX_NEW)
    assert [dec.generate(p, LC.MAX_NEW) for p in ps] == exp              # a plain generate() after lookup runs


def test_limits_and_callbacks(tmp_path):
    base, seed = _greedy_case("llama-4")
    dec, t, cfg = _llama(tmp_path, base, seed)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(seed, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    p, e = ps[0], exp[0]
    cuts, inside, pos = (0, 1, 2, 4, 5, 9, 12), set(), 1
    for _, a in LK.simulate(p, e):   # a step emits e[pos .. pos + a]: a cut inside keeps some of an accepted run and discards the rest
        inside |= {m for m in cuts if pos < m < pos + a + 1}
        pos += a + 1
    assert {2, 4, 12} <= inside, "precondition: cuts fall inside accepted runs"
    for m in cuts:
        got, st = dec.generate_lookup(p, m)
        assert got == e[:m], m
        assert st["verify_steps"] == (0 if m <= 1 else len(LK.simulate(p, e[:m]))), m
    seen = []
    got, _ = dec.generate_lookup(p, LC.MAX_NEW, on_token=lambda tok: seen.append(tok) or len(seen) < 3)
    assert got == seen == e[:3]
    seen = []
    got, _ = dec.generate_lookup(p, LC.MAX_NEW, on_token=seen.append)     # (None: go on) bursts of 4 steps
    assert got == seen == e


# ---- 5. stops and the end of the cache ---------------------------------------------------------------------------------------

def test_stop_ids(tmp_path):
    dec, t, cfg = _llama(tmp_path, LC.EOS_BASE, LC.EOS_SEED)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(LC.EOS_SEED, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    ends = LC.stop_steps(orc, ps, LC.MAX_NEW)
    assert len(ends) >= 2 and len(set(ends.values())) >= 2 and min(ends.values()) == 0, ends   # one prompt ends at once
    for p, e in zip(ps, exp):
        got, _ = dec.generate_lookup(p, LC.MAX_NEW)
        assert got == e and all(tok not in cfg["eos_token_id"] for tok in got)
    # an explicit list overrides the config's: the run goes through the config's ids and ends before `stop`
    # an explicit list overrides the config's: with [2] alone the runs go through the config's other ids
    long_orc = L.LlmOracle(t, dict(cfg, eos_token_id=[2]))
    stopped = sorted(ends)
    free, gap = LC.oracle_runs(long_orc, [ps[i] for i in stopped], LC.MAX_NEW)
    assert gap >= LC.GAP and all(len(f) > len(exp[i]) for f, i in zip(free, stopped))
    for f, i in zip(free, stopped):
        assert dec.generate_lookup(ps[i], LC.MAX_NEW, stop_ids=[2])[0] == f
        assert dec.generate_lookup(ps[i], LC.MAX_NEW, stop_ids=[2, f[-1]])[0] == f[:f.index(f[-1])]


def test_the_end_of_the_cache(tmp_path):
    base, seed = _greedy_case("llama-4")
    dec, t, cfg = _llama(tmp_path, base, seed, max_context=48)
    assert dec.context == 48
    orc = L.LlmOracle(t, cfg)
    p45 = np.random.default_rng(seed + 100).integers(4, cfg["vocab_size"], 45).tolist()
    p40 = np.random.default_rng(seed + 101).integers(4, cfg["vocab_size"], 40).tolist()
    (e45, e40), gap = LC.oracle_runs(orc, [p45, p40], LC.MAX_NEW, context_limit=48)
    assert gap >= LC.GAP and len(e45) == 3 and len(e40) == 8
    got, st = dec.generate_lookup(p45, LC.MAX_NEW)
    assert got == e45 and dec.cache_len() <= 48
    assert st["verify_steps"] + st["single_row_steps"] >= 1
    for D in (7, 2):   # 8-row steps cannot all fit: the steps get narrower, down to one row
        got, st = dec.generate_lookup(p40, LC.MAX_NEW, draft_tokens=D)
        assert got == e40 and dec.cache_len() <= 48, D
    assert dec.generate(p40, LC.MAX_NEW) == e40


# ---- 6. the other stacks -----------------------------------------------------------------------------------------------------

def test_gpt2_lookup_equals_float64_greedy(tmp_path):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(**G.SMALL)
    d = str(tmp_path / "gpt2")
    _, t = G.gpt2_model(d, cfg, seed=1)
    dec, ref = HipDecoder(d, 0), _Gpt264(t, cfg)
    for p in LC.prompts(1, cfg["vocab_size"], n=5, lo=1, hi=39):
        want, gap = _trace64(ref, p, 24)
        assert gap >= LC.GAP, f"precondition: {gap:.2e}"
        if G.ENDOFTEXT in want:
            want = want[:want.index(G.ENDOFTEXT)]
        for D in (7, 3):
            got, st = dec.generate_lookup(p, 24, draft_tokens=D, stop_ids=[G.ENDOFTEXT])
            assert got == want, (len(p), D)
        assert dec.generate_lookup(p, 24)[0] == dec.generate(p, 24) == want  # config.json's eos id is the same


def test_gguf_q8_0_q4_k_lookup_equals_the_oracle(tmp_path):
    from kjarni_amd import HipDecoder
    path, twin = str(tmp_path / "m" / "model.gguf"), str(tmp_path / "twin")
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    cfg, hf = GG.gguf_model(path, GG.LLAMA_Q, types, seed=3, rope_freqs=True, twin=twin)
    dec = HipDecoder(str(tmp_path / "m"))
    by = dec.weight_bytes_by_type()
    assert by.get("Q8_0", 0) > 0 and by.get("Q4_K", 0) > 0
    orc = L.LlmOracle(hf, cfg)
    ps = LC.prompts(7, cfg["vocab_size"], n=5)
    exp, gap = LC.oracle_runs(orc, ps, 24)
    assert gap >= LC.GAP, f"precondition: {gap:.2e}"
    for p, e in zip(ps, exp):
        got, st = dec.generate_lookup(p, 24)
        assert got == e == dec.generate(p, 24), len(p)
        assert st["verify_steps"] >= 1
    assert dec.verify_gemv_calls() == (0, 0)                              # quantized matrices never take the f32 / bf16 GEMVs


# ---- 7. the Generator --------------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


@pytest.fixture(scope="module")
def gpt2_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lookup") / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    return d, cfg, t


def test_generator_prompt_lookup(gpt2_dir):
    from kjarni_amd import BpeTokenizer, Generator
    from kjarni_amd.chat import GenerationConfig
    d, cfg, t = gpt2_dir
    gen = Generator("gpt2", model_path=d)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    ref = Gpt2Ref64(t, cfg)
    greedy = GenerationConfig(do_sample=False, max_new_tokens=30)
    want = ["".join(tok.decode([i], skip_special=False) for i in ref.greedy(gen.encode(text), 30, stop=(G.ENDOFTEXT,))) for text in TEXTS]
    assert [gen.generate(text, greedy) for text in TEXTS] == want and gen.verify_gemv_calls() == (0, 0)
    gen.set_prompt_lookup(7)
    assert [gen.generate(text, greedy) for text in TEXTS] == want
    moved = gen.verify_gemv_calls()
    assert sum(moved) > 0                                                 # the lookup loop ran
    for text, w in zip(TEXTS, want):
        pieces = []
        gen.stream(text, lambda s: pieces.append(s) or True, greedy)
        assert "".join(pieces) == w
    # a config with a repetition penalty is not applicable: the plain path, whatever the setting
    gen.set_prompt_lookup(0)
    pen = GenerationConfig(do_sample=False, max_new_tokens=30, repetition_penalty=1.3)
    plain = [gen.generate(text, pen) for text in TEXTS]
    before = gen.verify_gemv_calls()
    gen.set_prompt_lookup(7)
    assert [gen.generate(text, pen) for text in TEXTS] == plain and gen.verify_gemv_calls() == before
    gen.set_prompt_lookup(0)                                              # off again: the plain path
    assert [gen.generate(text, greedy) for text in TEXTS] == want and gen.verify_gemv_calls() == before
    with pytest.raises(Exception, match="draft_tokens"):
        gen.set_prompt_lookup(8)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------

def test_errors(tmp_path):
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    base, seed = _greedy_case("llama-4")
    dec, t, cfg = _llama(tmp_path, base, seed, max_context=48)
    seen = []
    for kw, field in ((dict(draft_tokens=0), "draft_tokens"), (dict(draft_tokens=8), "draft_tokens"), (dict(ngram_max=5), "ngram_max"),
                      (dict(ngram_max=0), "ngram_max"), (dict(ngram_min=0), "ngram_min"), (dict(ngram_max=2, ngram_min=3), "ngram_min")):
        with pytest.raises(KjarniException, match=field) as e:
            dec.generate_lookup([5, 6, 7], 4, on_token=seen.append, **kw)
        assert e.value.code == E.INVALID_CONFIG and seen == []
        with pytest.raises(KjarniException, match=field) as e:
            ops.lookup_draft([5, 6, 5], **kw)
        assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(KjarniException, match="context") as e:            # a prompt longer than the context
        dec.generate_lookup(list(range(4, 4 + 49)), 4, on_token=seen.append)
    assert e.value.code == E.INVALID_CONFIG and seen == []
    with pytest.raises(KjarniException, match="empty prompt"):
        dec.generate_lookup([], 4)
    dec.reset()
    dec.forward(list(range(4, 4 + 42)), fetch=False)
    for draft, rows in (([5, 6, 7], 3), ([5, 6, 7], 9), ([5], 0)):
        with pytest.raises(KjarniException, match="rows") as e:
            dec.verify_step(4, draft, rows)
        assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(KjarniException, match="context") as e:            # 42 + 7 rows > 48
        dec.verify_step(4, [5, 6], 7)
    assert e.value.code == E.INVALID_CONFIG and dec.cache_len() == 42
    picks, a, _ = dec.verify_step(4, [5, 6], 6)                          # 42 + 6 rows == 48 fits
    assert len(picks) == a + 1 and dec.cache_len() == 42 + a + 1
