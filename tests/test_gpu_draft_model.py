"""Speculative decoding with a draft model on the GPU (kjarni_hip_decoder_generate_draft, kjarni_hip_decoder_draft_round and
the Generator / Chat setters).

Single rounds against float64 (the drafter's proposals, the target's picks, every logits row, both caches, the invariant on
the two cache lengths, a round after a full acceptance); the greedy loop against the oracle's ids with three drafters (the
target's own checkpoint, another seed, the target's tensors plus noise) and its stats against tests/draft_cases.simulate;
the sampled loop against generate_sampled without lookup for the same draws; other stacks; limits; refusals; the graph key
after a drafter was freed; Generator and Chat.  Float bar: the decoder's, max |gpu - ref| <= 1e-4 * max(1, max |ref|).
Token comparisons carry the precondition that the reference's two best logits are >= LC.GAP apart, asserted here.

The case builders touch no GPU, so every precondition can be evaluated anywhere."""
import os
import shutil

import numpy as np
import pytest

from oracle import llm_oracle as L
from tests import draft_cases as DC
from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import llm_ref64, qwen3_fixture as Q3, synth
from tests.gpt2_ref64 import Gpt2Ref64
from tests.qwen3_ref64 import Qwen3Ref64, assert_margins

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROUND_LENS = (1, 7, 8, 23, 24, 40)     # both prompt routes (the matrix-core route starts at 24 rows)
ROUND_ROWS = (2, 3, 5, 8)
AHEAD = 17                             # the first pick and two rounds of up to 8 tokens
NOISE, NOISE_SEED = 1.0, 100
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ZERO = dict(verify_steps=0, drafted_tokens=0, accepted_tokens=0, single_row_steps=0)


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _within(got, ref, what):
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), _bar(ref)
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


# ---- float64 references with every row's logits (as tests/test_gpu_lookup.py states them) --------------------------------------

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


def _gap(row):
    top = np.partition(np.asarray(row, np.float64), -2)[-2:]
    return float(top[1] - top[0])


def _trace64(ref, prompt, n):
    """n greedy tokens of the float64 reference (last maximum wins) and the smallest gap between its two best logits."""
    cache = ref.new()
    row = ref.logits(prompt, cache)[-1]
    out, gap = [], float("inf")
    for _ in range(n):
        gap = min(gap, _gap(row))
        out.append(_last_max(row))
        row = ref.logits([out[-1]], cache)[-1]
    return out, gap


def _truncate64(cache, keep):
    return [(k[:keep], v[:keep]) for k, v in cache]


def _check_cache(dec, ref_cache, what):
    assert dec.cache_len() == ref_cache[0][0].shape[0], what
    got = [dec.kv_rows(i) for i in range(len(ref_cache))]
    for (layer, name), (err, bar) in llm_ref64.cache_errors(got, ref_cache).items():
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e}"


def _noisy(t, noise=NOISE, seed=NOISE_SEED):
    """The tensors plus noise x each 2-D tensor's std, drawn from default_rng(seed) in the dict's order."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in t.items():
        out[k] = (v + np.float32(noise * float(v.std())) * rng.standard_normal(v.shape).astype(np.float32)).astype(np.float32) if v.ndim == 2 else v
    return out


def _llama(tmp_path, base, seed, tag="", **kw):
    import kjarni_amd
    d = str(tmp_path / f"{base['model_type']}-{seed}{tag}")
    ctx = kw.pop("max_context", 0)
    cfg, t = synth.llm_model(d, base, seed=seed, **kw)
    return kjarni_amd.HipDecoder(d, max_context=ctx), t, cfg


def _from_tensors(tmp_path, name, cfg, t, max_context=0):
    import kjarni_amd
    d = synth.write_model_dir(str(tmp_path / name), cfg, t)
    return kjarni_amd.HipDecoder(d, max_context=max_context)


def _three_drafters(tmp_path, base, seed, t, cfg, max_context=0):
    """{name: (decoder, tensors)}: (i) the target's checkpoint loaded a second time, (ii) another seed, (iii) the target's tensors
    plus noise."""
    other, t_other, _ = _llama(tmp_path, base, seed + 1000, tag="-other", max_context=max_context)
    t_noisy = _noisy(t)
    return {"same": (_from_tensors(tmp_path, "same", cfg, t, max_context), t),
            "other": (other, t_other),
            "noisy": (_from_tensors(tmp_path, "noisy", cfg, t_noisy, max_context), t_noisy)}


def _invariant(dec, drf, what):
    assert dec.cache_len() - 1 <= drf.cache_len() <= dec.cache_len(), f"{what}: target {dec.cache_len()} drafter {drf.cache_len()}"


# ---- 1. rounds against float64 -------------------------------------------------------------------------------------------------

def _round_cases(ref, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for n in ROUND_LENS:
        prompt = rng.integers(ref.first_id, ref.vocab, n).tolist()
        cont, gap = _trace64(ref, prompt, AHEAD)
        assert gap >= LC.GAP, f"precondition: prompt of {n}: the reference's two best logits come within {gap:.2e}"
        cases.append((prompt, cont))
    return cases


def _one_round(dec, drf, ref, dref, hist, cache, rows, cont_at, cont, what):
    """One round on the history `hist` (its last token in neither cache; `cache`: the target reference's, holding hist[:-1]).
    Returns (a, drafter proposals compared or not)."""
    before = dec.cache_len()
    assert before == len(hist) - 1
    proposals, picks, a, logits = dec.draft_round(drf, hist[-1], rows)
    assert len(proposals) == rows - 1 and len(picks) == a + 1 and logits.shape == (rows, ref.vocab), what
    # the drafter's proposals: its reference's greedy continuation of the history, compared where that reference clears GAP
    dcache = dref.new()
    row = dref.logits(hist, dcache)[-1]
    want_d, dgap = [], float("inf")
    for i in range(rows - 1):
        dgap = min(dgap, _gap(row))
        want_d.append(_last_max(row))
        if i + 1 < rows - 1:
            row = dref.logits([want_d[-1]], dcache)[-1]
    compared = dgap >= LC.GAP
    if compared:
        assert proposals == want_d, what
    # every logits row: the target's output after the token and the proposals as made
    want = ref.logits([hist[-1]] + proposals[:rows - 1], list(cache))
    for i in range(rows):
        _within(logits[i], want[i], f"{what}: logits row {i}")
    # the picks are the target's own greedy tokens (on its greedy path: the precondition of _round_cases covers them)
    want_a = 0
    while want_a < rows - 1 and proposals[want_a] == cont[cont_at + want_a]:
        want_a += 1
    assert a == want_a and picks == cont[cont_at:cont_at + a + 1], what
    assert dec.cache_len() == before + a + 1, what
    _invariant(dec, drf, what)
    assert drf.cache_len() == (dec.cache_len() if a < rows - 1 else dec.cache_len() - 1), what
    ref.logits([hist[-1]] + picks[:a], cache)
    return a, compared


@pytest.mark.parametrize("base", [synth.LLAMA_TEST, synth.QWEN_TEST], ids=["llama-gqa-rope-scaling", "qwen2-bias-mqa-untied"])
def test_rounds_against_float64(tmp_path, base):
    dec, t, cfg = _llama(tmp_path, base, 3)
    ref = _Llama64(t, cfg)
    drafters = _three_drafters(tmp_path, base, 3, t, cfg)
    cases = _round_cases(ref, 0 if base is synth.LLAMA_TEST else 1)
    compared = {k: 0 for k in drafters}
    for name, (drf, dt) in drafters.items():
        dref = _Llama64(dt, cfg)
        for prompt, cont in cases:
            pcache = ref.new()
            ref.logits(prompt, pcache)
            for rows in ROUND_ROWS:
                what = f"drafter {name} prompt {len(prompt)} rows {rows}"
                dec.reset()
                dec.forward(prompt, fetch=False)
                drf.reset()
                drf.forward(prompt, fetch=False)
                cache = list(pcache)
                hist = list(prompt) + cont[:1]
                a1, c1 = _one_round(dec, drf, ref, dref, hist, cache, rows, 1, cont, what + " round 1")
                if name == "same":
                    assert a1 == rows - 1, what                              # the case the 2-row pass exists for
                hist = hist + cont[1:a1 + 2]
                a2, c2 = _one_round(dec, drf, ref, dref, hist, cache, rows, a1 + 2, cont, what + " round 2")
                compared[name] += int(c1) + int(c2)
                # afterwards: every cache row of the target, and every row the drafter claims, against float64
                _check_cache(dec, cache, what)
                held = dec.resident()[:drf.cache_len()]
                assert drf.resident() == held and len(held) == drf.cache_len(), what
                dcache = dref.new()
                dref.logits(held, dcache)
                _check_cache(drf, dcache, what + " (drafter)")
    assert all(n >= len(cases) * len(ROUND_ROWS) for n in compared.values()), compared   # most proposals were compared


# ---- 2. the loop == the oracle ---------------------------------------------------------------------------------------------------

def _oracle_drafter(t, cfg):
    return DC.ModelDrafter(_Llama64(t, cfg), _truncate64)


@pytest.mark.parametrize("name", sorted(LC.GREEDY_MODELS))
def test_loop_equals_the_oracle(tmp_path, name):
    base, seed = LC.GREEDY_MODELS[name]
    dec, t, cfg = _llama(tmp_path, base, seed)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(seed, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP, f"precondition: the oracle's two best logits come within {gap:.2e}"
    drafters = _three_drafters(tmp_path, base, seed, t, cfg)
    sims = None
    if name == "llama-7":   # the noisy drafter's rounds, re-derived: full misses, partial acceptances and full acceptances all occur
        sims = [DC.simulate(e, _oracle_drafter(drafters["noisy"][1], cfg), p, 7) for p, e in zip(ps[:6], exp[:6])]
        dgap = min(g for _, g in sims)
        assert dgap >= LC.GAP, f"precondition: the noisy drafter's two best logits come within {dgap:.2e}"
        accepted = [a for log, _ in sims for _, a in log]
        assert any(a == 0 for a in accepted) and any(0 < a < 7 for a in accepted) and any(a == 7 for a in accepted), accepted
    for dname, (drf, dt) in drafters.items():
        for D in (1, 4, 7):
            for i, (p, e) in enumerate(zip(ps, exp)):
                got, st = dec.generate_draft(drf, p, LC.MAX_NEW, D)
                what = (dname, D, len(p))
                assert got == e, what
                _invariant(dec, drf, what)
                assert st["single_row_steps"] == 0 and st["drafted_tokens"] == D * st["verify_steps"], what
                assert st["accepted_tokens"] + st["verify_steps"] >= len(got) - 1, what
                if dname == "same" and len(e) == LC.MAX_NEW:
                    # every round but the run's last accepts its whole draft
                    rounds = -(-(len(e) - 1) // (D + 1))
                    assert st["verify_steps"] == rounds and st["accepted_tokens"] >= (rounds - 1) * D, what
                if dname == "noisy" and D == 7 and sims is not None and i < 6 and len(e) == LC.MAX_NEW:
                    log = sims[i][0]
                    assert st["verify_steps"] == len(log), what
                    body = sum(a for _, a in log[:-1])
                    assert body + log[-1][1] <= st["accepted_tokens"] <= body + log[-1][0], what
    # a plain generate() on the target and on the drafters afterwards gives their oracles' ids
    assert [dec.generate(p, LC.MAX_NEW) for p in ps] == exp
    for dname in ("other", "noisy"):
        drf, dt = drafters[dname]
        dexp, dgap = LC.oracle_runs(L.LlmOracle(dt, cfg), ps[:3], 12)
        if dgap >= LC.GAP:
            assert [drf.generate(p, 12) for p in ps[:3]] == dexp, dname


# ---- 3. sampled ----------------------------------------------------------------------------------------------------------------

SAMPLING = dict(temperature=0.8, top_k=40, top_p=0.95)


def test_sampled_equals_the_plain_loop_for_the_same_draws(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    drafters = _three_drafters(tmp_path, base, seed, t, cfg)
    ps = LC.prompts(seed, cfg["vocab_size"])[:5]
    rng = np.random.default_rng(77)
    n = 24
    for penalty in (1.0, 1.3):
        for p in ps:
            # exactly n draws for n tokens: a loop that took a draw for a row it does not decide would exhaust the stream
            u = rng.random(n).astype(np.float32).tolist()
            plain, st0 = dec.generate_sampled(p, n, lookup=None, uniforms=u, repetition_penalty=penalty, **SAMPLING)
            assert st0 == ZERO
            for dname in ("same", "other"):
                drf = drafters[dname][0]
                for D in (3, 7):
                    got, st = dec.generate_draft(drf, p, n, D, sample=True, uniforms=u, repetition_penalty=penalty, **SAMPLING)
                    what = (dname, D, penalty, len(p))
                    assert got == plain, what
                    assert st["verify_steps"] >= 1 and st["drafted_tokens"] == D * st["verify_steps"], what
                    _invariant(dec, drf, what)
    # (the stream's position after a call: test_generator_with_a_draft_model runs calls back to back on one seeded generator)
    # the same drafter that always agrees in greedy mode accepts under sampling wherever the draw picks the arg-max: with
    # top_k = 1 every draft of the same checkpoint is accepted
    p = ps[0]
    u = [0.5] * 24
    got, st = dec.generate_draft(drafters["same"][0], p, 24, 7, sample=True, uniforms=u, top_k=1)
    assert got == dec.generate_sampled(p, 24, lookup=None, uniforms=u, top_k=1)[0]
    assert st["accepted_tokens"] >= 7 * (st["verify_steps"] - 1)


def test_requests_the_draft_loops_do_not_take(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    drf = _llama(tmp_path, base, seed + 1000, tag="-other")[0]
    p = LC.prompts(seed, cfg["vocab_size"])[0]
    before = dec.verify_gemv_calls()
    drf.reset()
    got, st = dec.generate_draft(drf, p, 12, 7, repetition_penalty=1.3)       # greedy with a penalty
    assert st == ZERO and got == dec.generate(p, 12, repetition_penalty=1.3)
    got, st = dec.generate_draft(drf, p, 12, 7, no_repeat_ngram=2)            # an n-gram ban, greedy
    assert st == ZERO and got == dec.generate(p, 12, no_repeat_ngram=2)
    u = [0.5] * 12
    got, st = dec.generate_draft(drf, p, 12, 7, sample=True, uniforms=u, no_repeat_ngram=2, **SAMPLING)   # ... and sampled
    assert st == ZERO and got == dec.generate_sampled(p, 12, lookup=None, uniforms=u, no_repeat_ngram=2, **SAMPLING)[0]
    assert dec.verify_gemv_calls() == before and drf.cache_len() == 0         # no verify step ran, the drafter was not touched


# ---- 4. other stacks -----------------------------------------------------------------------------------------------------------

def test_qwen2_drafts_for_llama(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    drf, _, dcfg = _llama(tmp_path, synth.QWEN_TEST, 5, vocab_size=cfg["vocab_size"], max_position_embeddings=cfg["max_position_embeddings"])
    assert dcfg["model_type"] == "qwen2" and drf.context == dec.context
    ps = LC.prompts(seed, cfg["vocab_size"])[:5]
    exp, gap = LC.oracle_runs(L.LlmOracle(t, cfg), ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    for p, e in zip(ps, exp):
        for D in (2, 7):
            got, st = dec.generate_draft(drf, p, LC.MAX_NEW, D)
            assert got == e and st["verify_steps"] >= 1, (D, len(p))
            _invariant(dec, drf, (D, len(p)))


def test_gpt2_drafts_for_gpt2(tmp_path):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(**G.SMALL)
    d, dd, ds = str(tmp_path / "gpt2"), str(tmp_path / "gpt2-draft"), str(tmp_path / "gpt2-same")
    _, t = G.gpt2_model(d, cfg, seed=1)
    G.gpt2_model(dd, cfg, seed=2)
    G.gpt2_model(ds, cfg, seed=1)
    dec, ref = HipDecoder(d, 0), _Gpt264(t, cfg)
    other, same = HipDecoder(dd, 0), HipDecoder(ds, 0)
    for p in LC.prompts(1, cfg["vocab_size"], n=4, lo=1, hi=39):
        want, gap = _trace64(ref, p, 24)
        assert gap >= LC.GAP, f"precondition: {gap:.2e}"
        if G.ENDOFTEXT in want:
            want = want[:want.index(G.ENDOFTEXT)]
        for drf in (other, same):
            for D in (7, 3):
                got, st = dec.generate_draft(drf, p, 24, D, stop_ids=[G.ENDOFTEXT])
                assert got == want, (len(p), D)
        if len(want) == 24:
            assert st["accepted_tokens"] >= 3 * (st["verify_steps"] - 1)        # (the last call: the same checkpoint, D = 3)


def test_qwen3_drafts_for_qwen3(tmp_path):
    from kjarni_amd import HipDecoder
    d, dd = str(tmp_path / "q3"), str(tmp_path / "q3-draft")
    cfg, t = Q3.qwen3_model(d, Q3.Q3_SMALL, seed=Q3.MODEL_SEED)
    Q3.qwen3_model(dd, Q3.Q3_SMALL, seed=Q3.MODEL_SEED + 1)
    dec, drf = HipDecoder(d, 0), HipDecoder(dd, 0)
    ref = Qwen3Ref64(t, cfg)
    prompt = Q3.seeded_prompt(Q3.GREEDY_PROMPT_SEED["Q3_SMALL"], cfg["vocab_size"], 9)
    want, gaps, tops = ref.greedy(prompt, 12)
    assert_margins(gaps, tops, "qwen3 target")
    assert cfg["eos_token_id"] not in want
    for D in (1, 4, 7):
        got, st = dec.generate_draft(drf, prompt, 12, D)
        assert got == want and st["verify_steps"] >= 1, D
        _invariant(dec, drf, D)
    assert dec.generate(prompt, 12) == want


def test_a_quantized_gguf_drafts_for_safetensors(tmp_path):
    from kjarni_amd import HipDecoder
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    path = str(tmp_path / "m" / "model.gguf")
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    qcfg, hf = GG.gguf_model(path, GG.LLAMA_Q, types, seed=3, rope_freqs=True)
    drf = HipDecoder(str(tmp_path / "m"))
    assert drf.weight_bytes_by_type().get("Q4_K", 0) > 0 and qcfg["vocab_size"] == cfg["vocab_size"] and drf.context >= dec.context
    ps = LC.prompts(seed, cfg["vocab_size"])[:4]
    exp, gap = LC.oracle_runs(L.LlmOracle(t, cfg), ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    for p, e in zip(ps, exp):
        got, st = dec.generate_draft(drf, p, LC.MAX_NEW, 4)
        assert got == e and st["verify_steps"] >= 1, len(p)
    # the drafter is still a working decoder of its own
    qexp, qgap = LC.oracle_runs(L.LlmOracle(hf, qcfg), ps[:2], 12)
    if qgap >= LC.GAP:
        assert [drf.generate(p, 12) for p in ps[:2]] == qexp


# ---- 5. limits -----------------------------------------------------------------------------------------------------------------

def _reaches_one_row(prompt, cont, drafter_oracle, D, cap):
    """The capacity rule on the host: does a run whose greedy continuation is `cont` reach a one-row step?  (The history fills
    the context with the cache one row short of it.)  Also the smallest drafter gap met."""
    hist, pos, cache, gap = list(prompt) + cont[:1], 1, len(prompt), float("inf")
    while len(hist) < cap:
        rows = min(D + 1, cap - cache)
        draft, g = drafter_oracle(hist, rows - 1)
        gap = min(gap, g)
        a = 0
        while a < rows - 1 and draft[a] == cont[pos + a]:
            a += 1
        hist += cont[pos:pos + a + 1]
        pos, cache = pos + a + 1, cache + a + 1
    return len(hist) == cap and cache == cap - 1, gap


def test_the_end_of_the_cache(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed, max_context=48)
    # an untied qwen2 drafter: these tiny tied checkpoints all tend to repeat the last token, which an unrelated tied drafter
    # proposes too, and a run that accepts whole drafts jumps over the one-row step
    drf, dt, dcfg = _llama(tmp_path, synth.QWEN_TEST, 5, vocab_size=cfg["vocab_size"], max_position_embeddings=cfg["max_position_embeddings"],
                           max_context=48)
    assert dec.context == 48 and drf.context == 48
    orc = L.LlmOracle(t, cfg)
    p45 = np.random.default_rng(seed + 100).integers(4, cfg["vocab_size"], 45).tolist()
    p40 = np.random.default_rng(seed + 103).integers(4, cfg["vocab_size"], 40).tolist()
    (e45, e40), gap = LC.oracle_runs(orc, [p45, p40], LC.MAX_NEW, context_limit=48)
    (cont,), gap2 = LC.oracle_runs(orc, [p40], 24)                            # the picks of rounds that reach past the context
    assert min(gap, gap2) >= LC.GAP and len(e45) == 3 and len(e40) == 8 and cont[:8] == e40
    got, st = dec.generate_draft(drf, p45, LC.MAX_NEW, 7)
    assert got == e45 and dec.cache_len() <= 48 and drf.cache_len() <= 48
    for D in (7, 2):   # 8-row rounds cannot all fit: the rounds get narrower, down to one row, which launches no drafter kernel
        reaches, dgap = _reaches_one_row(p40, cont, _oracle_drafter(dt, dcfg), D, 48)
        assert reaches and dgap >= LC.GAP, f"precondition: D = {D}: one row reached: {reaches}, drafter gap {dgap:.2e}"
        got, st = dec.generate_draft(drf, p40, LC.MAX_NEW, D)
        assert got == e40 and dec.cache_len() <= 48 and drf.cache_len() <= 48, D
        _invariant(dec, drf, D)
        assert st["single_row_steps"] > 0 and st["verify_steps"] >= 1, (D, st)
    # nothing was written at or past either capacity: both models still give their oracles' ids
    assert dec.generate(p40, LC.MAX_NEW) == e40
    short = p40[:9]
    dexp, dgap = LC.oracle_runs(L.LlmOracle(dt, dcfg), [short], 12)
    if dgap >= LC.GAP:
        assert drf.generate(short, 12) == dexp[0]


def test_stops_limits_and_callbacks(tmp_path):
    dec, t, cfg = _llama(tmp_path, LC.EOS_BASE, LC.EOS_SEED)
    drf = _from_tensors(tmp_path, "same", cfg, t)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(LC.EOS_SEED, cfg["vocab_size"])
    exp, gap = LC.oracle_runs(orc, ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    ends = LC.stop_steps(orc, ps, LC.MAX_NEW)
    assert len(ends) >= 2 and min(ends.values()) == 0, ends                   # one prompt ends at once
    for p, e in zip(ps, exp):
        got, _ = dec.generate_draft(drf, p, LC.MAX_NEW, 7)
        assert got == e and all(tok not in cfg["eos_token_id"] for tok in got)
    i = max(range(len(ps)), key=lambda j: len(exp[j]))
    p, e = ps[i], exp[i]
    assert len(e) >= 8
    assert dec.generate_draft(drf, p, LC.MAX_NEW, 7, stop_ids=[e[5]])[0] == e[:e.index(e[5])]   # an explicit stop id inside a round
    for m in (0, 1, 2, 5, 7):                                                   # max_new_tokens inside accepted runs
        assert dec.generate_draft(drf, p, m, 7)[0] == e[:m], m
    seen = []
    got, _ = dec.generate_draft(drf, p, LC.MAX_NEW, 7, on_token=lambda tok: seen.append(tok) or len(seen) < 3)
    assert got == seen == e[:3]
    seen = []
    got, _ = dec.generate_draft(drf, p, LC.MAX_NEW, 7, on_token=seen.append)
    assert got == seen == e


def test_prefix_reuse_on_both_models(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    drf = _llama(tmp_path, base, seed + 1000, tag="-other")[0]
    ps = LC.prompts(seed, cfg["vocab_size"])
    first = next(p for p in ps if len(p) >= 12)
    exp, gap = LC.oracle_runs(L.LlmOracle(t, cfg), [first], LC.MAX_NEW)
    assert gap >= LC.GAP
    second = first + exp[0][:6]                                                # the next turn of a conversation: a shared prefix
    exp2, gap2 = LC.oracle_runs(L.LlmOracle(t, cfg), [second], 16)
    assert gap2 >= LC.GAP and exp2[0] == exp[0][6:22]
    dec.set_prefix_reuse(True)
    drf.set_prefix_reuse(True)
    assert dec.generate_draft(drf, first, LC.MAX_NEW, 4)[0] == exp[0]
    r0, d0 = dec.prefix_stats(), drf.prefix_stats()
    assert dec.generate_draft(drf, second, 16, 4)[0] == exp2[0]
    r1, d1 = dec.prefix_stats(), drf.prefix_stats()
    assert r1[0] - r0[0] >= len(first) and d1[0] - d0[0] >= len(first)       # both kept the rows of the shared prefix
    assert r1[1] - r0[1] <= 7 and d1[1] - d0[1] <= 7


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed, max_context=48)
    ok = _llama(tmp_path, base, seed + 1000, tag="-other", max_context=48)[0]
    short = _llama(tmp_path, base, seed + 1001, tag="-short", max_context=40)[0]
    vocab = _llama(tmp_path, base, seed + 1002, tag="-vocab", vocab_size=cfg["vocab_size"] + 1, max_context=48)[0]
    dec.forward([5, 6, 7], fetch=False)
    ok.forward([5, 6], fetch=False)
    seen = []
    cases = [(None, dict(draft_tokens=4), [5, 6, 7], "draft"), (dec, dict(draft_tokens=4), [5, 6, 7], "draft"),
             (vocab, dict(draft_tokens=4), [5, 6, 7], "vocab"), (short, dict(draft_tokens=4), [5, 6, 7], "context"),
             (ok, dict(draft_tokens=0), [5, 6, 7], "draft_tokens"), (ok, dict(draft_tokens=8), [5, 6, 7], "draft_tokens"),
             (ok, dict(draft_tokens=4), [], "prompt"), (ok, dict(draft_tokens=4), list(range(4, 4 + 49)), "prompt")]
    for drf, kw, prompt, field in cases:
        with pytest.raises(KjarniException, match=field) as e:
            dec.generate_draft(drf, prompt, 4, on_token=seen.append, **kw)
        assert e.value.code == E.INVALID_CONFIG and seen == [], field
        assert dec.cache_len() == 3 and ok.cache_len() == 2, field            # before any GPU work: both caches untouched
    import kjarni_amd
    if kjarni_amd.device_count() > 1:                                          # another device (needs two)
        far = kjarni_amd.HipDecoder(str(tmp_path / f"{base['model_type']}-{seed + 1000}-other"), device=1, max_context=48)
        with pytest.raises(KjarniException, match="device") as e:
            dec.generate_draft(far, [5, 6, 7], 4, 4)
        assert e.value.code == E.INVALID_CONFIG
    # the test hook: rows, the drafter's resident tokens
    for rows in (1, 9):
        with pytest.raises(KjarniException, match="rows") as e:
            dec.draft_round(ok, 9, rows)
        assert e.value.code == E.INVALID_CONFIG
    ok.reset()
    ok.forward([5, 7], fetch=False)                                            # not the target's tokens
    with pytest.raises(KjarniException, match="draft") as e:
        dec.draft_round(ok, 9, 4)
    assert e.value.code == E.INVALID_CONFIG and dec.cache_len() == 3 and ok.cache_len() == 2
    ok.reset()
    ok.forward([5], fetch=False)                                               # too few rows
    with pytest.raises(KjarniException, match="draft"):
        dec.draft_round(ok, 9, 4)
    ok.forward([6], fetch=False)
    proposals, picks, a, _ = dec.draft_round(ok, 9, 4)                         # the target's tokens up to cache_len - 1: accepted
    assert len(proposals) == 3 and len(picks) == a + 1 and dec.cache_len() == 3 + a + 1


# ---- 7. lifetime: the graph key ------------------------------------------------------------------------------------------------

def test_a_new_drafter_after_the_old_one_was_freed(tmp_path):
    base, seed = LC.GREEDY_MODELS["llama-4"]
    dec, t, cfg = _llama(tmp_path, base, seed)
    ps = LC.prompts(seed, cfg["vocab_size"])[:4]
    exp, gap = LC.oracle_runs(L.LlmOracle(t, cfg), ps, LC.MAX_NEW)
    assert gap >= LC.GAP
    u = np.random.default_rng(3).random(LC.MAX_NEW).astype(np.float32).tolist()
    plain = dec.generate_sampled(ps[0], LC.MAX_NEW, lookup=None, uniforms=u, **SAMPLING)[0]
    for round_, dseed in enumerate((seed + 1000, seed + 2000, seed)):        # the allocator may hand the same addresses back
        drf = _llama(tmp_path, base, dseed, tag=f"-life{round_}")[0]
        for p, e in zip(ps, exp):
            assert dec.generate_draft(drf, p, LC.MAX_NEW, 7)[0] == e, (round_, len(p))
        assert dec.generate_draft(drf, ps[0], LC.MAX_NEW, 7, sample=True, uniforms=u, **SAMPLING)[0] == plain, round_
        del drf
    got, st = dec.generate_lookup(ps[0], LC.MAX_NEW)                          # the lookup rule after a drafter: its own chains
    assert got == exp[0]


# ---- 8. Generator and Chat -----------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small"]
LLAMA_SPECIAL = {"bos": 700, "eot": 704, "end_of_text": 701, "eom": 705}


def test_generator_with_a_draft_model(tmp_path):
    from kjarni_amd import Generator
    from kjarni_amd.chat import GenerationConfig
    d, dd = str(tmp_path / "gpt2"), str(tmp_path / "gpt2-draft")
    cfg = G.gpt2_config(**dict(G.SMALL, n_ctx=128))
    G.gpt2_model(d, cfg, seed=4, tokenizer=True)
    G.gpt2_model(dd, cfg, seed=5)
    gen = Generator("gpt2", model_path=d)
    configs = [GenerationConfig(do_sample=False, max_new_tokens=24), GenerationConfig(do_sample=True, top_k=50, max_new_tokens=24),
               GenerationConfig(do_sample=True, top_k=50, max_new_tokens=24, repetition_penalty=1.3)]
    gen.seed(11)
    plain = [gen.generate(text, c) for text in TEXTS for c in configs]
    assert gen.verify_gemv_calls() == (0, 0)
    gen.set_draft_model(dd, 4)
    gen.seed(11)
    assert [gen.generate(text, c) for text in TEXTS for c in configs] == plain
    moved = gen.verify_gemv_calls()
    assert sum(moved) > 0                                                       # the draft loops ran
    pieces = []
    gen.seed(11)
    gen.stream(TEXTS[0], lambda s: pieces.append(s) or True, configs[0])
    assert "".join(pieces) == plain[0]
    moved = gen.verify_gemv_calls()
    gen.set_draft_model(None, 0)                                                # freed: the old path
    gen.seed(11)
    assert [gen.generate(text, c) for text in TEXTS for c in configs] == plain and gen.verify_gemv_calls() == moved
    with pytest.raises(Exception, match="draft_tokens"):
        gen.set_draft_model(dd, 8)
    gen.set_draft_model(d, 7)                                                   # the model's own checkpoint as its drafter
    gen.seed(11)
    assert [gen.generate(text, c) for text in TEXTS for c in configs] == plain


def test_chat_with_a_draft_model(tmp_path):
    from kjarni_amd.chat import Chat, GenerationConfig
    d, dd = str(tmp_path / "llama"), str(tmp_path / "llama-draft")
    over = dict(vocab_size=720, bos_token_id=LLAMA_SPECIAL["bos"],
                eos_token_id=[LLAMA_SPECIAL["end_of_text"], LLAMA_SPECIAL["eom"], LLAMA_SPECIAL["eot"]])
    synth.llm_model(d, synth.LLAMA_TEST, seed=11, **over)
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    synth.llm_model(dd, synth.LLAMA_TEST, seed=12, **over)
    chat = Chat("llama3.2-1b-instruct", model_path=d)
    configs = [GenerationConfig(do_sample=False, max_new_tokens=16), GenerationConfig(do_sample=True, top_k=50, max_new_tokens=16)]
    chat.seed(7)
    plain = [chat.send(m, c) for m in ("Hello there.", "Count to three.") for c in configs]
    assert chat.verify_gemv_calls() == (0, 0)
    chat.set_draft_model(dd, 5)
    chat.seed(7)
    assert [chat.send(m, c) for m in ("Hello there.", "Count to three.") for c in configs] == plain
    moved = chat.verify_gemv_calls()
    assert sum(moved) > 0
    chat.set_draft_model(None, 0)
    chat.seed(7)
    assert [chat.send(m, c) for m in ("Hello there.", "Count to three.") for c in configs] == plain and chat.verify_gemv_calls() == moved
