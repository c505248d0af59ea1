"""Prompt-lookup decoding for sampled requests on the GPU (kjarni_hip_decoder_generate_sampled and its hooks).

The rows cut and the rows penalty alone (bit-exact where the contract says so); one sampled verify step against float64; the
loop against the plain sampled loop and against the float64 oracle's trace; limits; the per-row fall-back to the logits; the
Generator; errors.  Token comparisons carry the preconditions of tests/sampled_lookup_cases.py (filter decisions and draws
clear of their boundaries), built and asserted there and asserted again here on what each test uses."""
import math
import os

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import llm_ref64, synth
from tests import lookup_cases as LK
from tests import sampled_lookup_cases as S
from tests import token_select_cases as T

pytestmark = pytest.mark.gpu
TOL = 1e-4
SUM_TOL = 2e-5          # the one-row cut's bar on the device sum (tests/test_gpu_token_select.py)
MAIN = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05)
CUT_PARAMS = {"k40-p0.9-minp0.05": dict(top_k=40, top_p=0.9, min_p=0.05), "p0.9-minp0.05": dict(top_p=0.9, min_p=0.05),
              "k3000": dict(top_k=3000)}


def _within(got, ref, what):
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), TOL * max(1.0, float(np.abs(ref).max()))
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _sampling(params):
    return {k: params.get(k) for k in ("temperature", "top_k", "top_p", "min_p")} | {"repetition_penalty": params.get("repetition_penalty", 1.0)}


# ---- 1. the rows cut alone ---------------------------------------------------------------------------------------------------

def _cut_rows(vocab):
    """The rows a block is mixed from: peaked, flat (every logit within a bin of the maximum) and short-tailed (half a unit
    between neighbours in a seeded order: no filter set reaches further than its own count)."""
    rng = np.random.default_rng(vocab)
    steep = (-0.5 * rng.permutation(vocab)).astype(np.float32)
    return {"peaked": T.zipf_logits(vocab, 1.3), "flat": (0.05 * rng.standard_normal(vocab)).astype(np.float32), "steep": steep,
            "zipf2": T.zipf_logits(vocab, 2.0)[::-1].copy()}


def _needed(row, top_k=None, top_p=None, min_p=None, p_inflate=1.0):
    """token_select_cases.needed_distance for any row."""
    v = np.sort(row.astype(np.float64))[::-1]
    cum = np.cumsum(np.exp(v - v[0]))
    V, d = v.size, 0.0
    k_on = top_k is not None and top_k < V
    if k_on:
        d = max(d, v[0] - v[max(top_k, 1) - 1])
    if top_p is not None:
        j = int(np.searchsorted(cum, top_p * p_inflate * cum[-1], side="right"))
        d = max(d, v[0] - v[j] if j < V else math.inf)
    if min_p is not None and not k_on and top_p is None:
        d = max(d, math.log(1.0 / min_p) if min_p > 0.0 else math.inf)
    return float(d)


def _check_row(row, f, h, capacity, tag):
    """Items 1-6 of the one-row cut's contract (tests/test_gpu_token_select.py, _check_call) for one row of a block."""
    V = row.size
    assert h["mx"] == row.max(), tag                                                        # 1
    v64 = row.astype(np.float64)
    want_sum = math.fsum(np.exp(v64 - v64.max()))
    err = abs(float(h["sum"]) - want_sum) / want_sum
    print(f"{tag}: sum rel err {err:.3e} count {h['count']} overflow {h['overflow']}")
    assert err <= SUM_TOL, (tag, err)                                                       # 2
    no_cut = T.no_cut_exists(V, **f)
    assert not no_cut
    if h["floor"] == -np.inf:    # a cut the histogram cannot place (it covers 64 below the maximum): reported, nothing appended
        assert _needed(row, **f) > 64.0 - 0.25, tag
        assert (h["count"], h["overflow"], h["ids"].size) == (V, 1, 0) and (h["slots"] == 0xFFFFFFFF).all(), tag
        return
    members = np.flatnonzero(row >= h["floor"])
    assert h["count"] == members.size, (tag, h["count"], members.size)                      # 3 / 4
    assert h["overflow"] == int(members.size > capacity), tag                               # 4
    ids = h["ids"].astype(np.int64)
    assert ids.size == min(members.size, capacity), tag
    assert np.unique(ids).size == ids.size and (ids < V).all(), tag
    assert np.array_equal(h["logits"], row[ids]), tag
    if not h["overflow"]:
        assert np.array_equal(np.sort(ids), members), tag
    else:
        assert np.isin(ids, members).all(), tag
    reach = float(h["mx"]) - float(h["floor"])
    assert reach >= _needed(row, **f), tag                                                  # 5
    assert reach <= _needed(row, p_inflate=1.001, **f) + 0.5, tag                           # 6
    # the slots behind the row's own candidates, up to its capacity, were never written (0xffffffff from the entry)
    assert (h["slots"][ids.size:] == 0xFFFFFFFF).all(), tag


@pytest.mark.parametrize("vocab", [257, 2049, 50257, 128256])
@pytest.mark.parametrize("name", sorted(CUT_PARAMS))
def test_rows_cut(name, vocab):
    """Blocks mixed from rows of this file's own making (_cut_rows: token_select_cases.sampler_logits has fixed vocabularies, the
    issue's four are needed here), each checked against the one-row contract with references that do not come from the kernel
    (float64 fsum, membership by comparison) and bit for bit against the one-row launcher on that row alone.  "The flat row
    overflows alone" is asserted where it can hold: vocabularies above the capacity of 4096, and not for k3000, whose 3000
    tokens plus two bins may pass 4096 on other rows too (there the per-row contract alone decides)."""
    from kjarni_amd import ops
    f = CUT_PARAMS[name]
    src = _cut_rows(vocab)
    order = ["peaked", "flat", "steep", "zipf2", "peaked", "steep", "flat", "zipf2"]
    alone = {k: ops.sample_candidates([v], capacity=4096, **f)[0] for k, v in src.items()}   # the one-row launcher, each row alone
    for rows in (1, 2, 5, 8):
        for pad in (0, 3):
            names = order[:rows] if rows > 1 else ["flat"]
            block = np.full((rows, vocab + pad), np.float32(1e30))                           # padding that would win any maximum
            for r, k in enumerate(names):
                block[r, :vocab] = src[k]
            for capacity in ((4096, 64) if (rows, pad) == (5, 3) else (4096,)):
                heads = ops.sample_candidates_rows(block, vocab=vocab, capacity=capacity, **f)
                overflowed = []
                for r, (k, h) in enumerate(zip(names, heads)):
                    tag = (name, vocab, rows, pad, capacity, r, k)
                    _check_row(src[k], f, h, capacity, tag)
                    one = alone[k]
                    assert h["mx"].tobytes() == one["mx"].tobytes() and h["sum"].tobytes() == one["sum"].tobytes(), tag
                    assert h["floor"] == one["floor"] and h["count"] == one["count"], tag
                    overflowed.append(k if h["overflow"] else None)
                if capacity == 4096 and vocab > 4096 and name != "k3000":
                    assert {k for k in overflowed if k} == ({"flat"} & set(names)), (name, vocab, rows, overflowed)   # the flat row, alone
                if capacity == 64:
                    assert any(overflowed) and all(h["count"] > 64 for h in heads if h["overflow"])


# ---- 2. the rows penalty alone -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vocab", [63, 50257])
def test_rows_penalty(vocab):
    from kjarni_amd import ops
    from kjarni_amd.chat import logits_process
    rng = np.random.default_rng(vocab)
    history = rng.integers(0, vocab, 40).tolist() + [5, 5, 9, 5]               # 5 three times, 9 once
    fresh = [t for t in range(vocab) if t not in history][:3]                  # tokens new to the history
    cases = [[5, 9, fresh[0], fresh[0], 5, fresh[1], fresh[0]],                # in the history, new, repeated new, repeated old
             [fresh[2]] * 7, [], [history[0], vocab + 7, fresh[1]]]            # one token seven times; rows = 1; an id both sides ignore
    for penalty in (1.1, 1.3, 0.8):
        for draft in cases:
            rows = len(draft) + 1
            for pad in (0, 3):
                block = np.full((rows, vocab + pad), np.float32(7.0))
                block[:, :vocab] = (3.0 * rng.standard_normal((rows, vocab))).astype(np.float32)      # mixed signs
                block[:, 5] = np.float32(-2.5)
                ids = [history[-1]] + draft
                got = ops.repetition_penalty_rows(block, ids, history, penalty, vocab=vocab)
                for r in range(rows):
                    want = logits_process(block[r, :vocab], history + ids[1:r + 1], repetition_penalty=penalty)
                    assert np.array_equal(got[r, :vocab], want), (vocab, penalty, draft, pad, r)
                assert np.array_equal(got[:, vocab:], block[:, vocab:])                            # the padding is not touched


# ---- models --------------------------------------------------------------------------------------------------------------------

HD64 = dict(synth.LLAMA_TEST, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512, head_dim=64,
            num_hidden_layers=1)


def _llama(tmp_path, base, seed, sharp=1.0, **kw):
    """(decoder, float64 reference) of a synthetic Llama-layout model, its logits multiplied by `sharp`."""
    import kjarni_amd
    from safetensors.numpy import save_file
    d = str(tmp_path / f"{base['model_type']}-{seed}-{sharp}")
    ctx = kw.pop("max_context", 0)
    cfg, t = synth.llm_model(d, base, seed=seed, **kw)
    if sharp != 1.0:
        t = S.sharpen(t, sharp)
        save_file({k: np.ascontiguousarray(v) for k, v in t.items()}, os.path.join(d, "model.safetensors"))
    return kjarni_amd.HipDecoder(d, max_context=ctx), S.Llama64(t, cfg), cfg


def _gpt2(tmp_path, seed=1):
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(**G.SMALL)
    d = str(tmp_path / "gpt2")
    _, t = G.gpt2_model(d, cfg, seed=seed)
    return HipDecoder(d, 0), S.Gpt264(t, cfg), cfg


def _gguf(tmp_path):
    from kjarni_amd import HipDecoder
    path = str(tmp_path / "m" / "model.gguf")
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    cfg, hf = GG.gguf_model(path, GG.LLAMA_Q, types, seed=3, rope_freqs=True, twin=str(tmp_path / "twin"))
    dec = HipDecoder(str(tmp_path / "m"))
    by = dec.weight_bytes_by_type()
    assert by.get("Q8_0", 0) > 0 and by.get("Q4_K", 0) > 0
    return dec, S.Llama64(hf, dict(cfg, model_type="llama")), cfg


def _prompts(seed, ref, n=8):
    """Seeded prompts with repeats, so that a lookup run drafts from the first step on."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        a = rng.integers(ref.first_id, ref.vocab, 5).tolist()
        yield a + a[:4] + rng.integers(ref.first_id, ref.vocab, 2).tolist() + a[:2]


def _distinct_prompts(seed, ref, n=64, length=11):
    """Seeded prompts without a repeated token (the largest penalty factor stays small)."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        yield (ref.first_id + rng.choice(ref.vocab - ref.first_id, length, replace=False)).tolist()


def _eos(cfg):
    e = cfg.get("eos_token_id", [])
    return tuple(e) if isinstance(e, (list, tuple)) else (e,)


def _trace(ref, cfg, params, n_new, seed, **kw):
    """The first seeded prompt on which the oracle's steered trace meets every precondition: (prompt, trace)."""
    why = None
    for prompt in _prompts(seed, ref):
        try:
            return prompt, S.build_trace(ref, prompt, n_new, params, avoid=_eos(cfg), **kw)
        except AssertionError as e:
            why = e
    raise AssertionError(f"precondition: none of the seeded prompts gives a clear trace ({why})")


# ---- 3. one sampled verify step against float64 ------------------------------------------------------------------------------

def _check_cache(dec, ref_cache, what):
    assert dec.cache_len() == ref_cache[0][0].shape[0], what
    got = [dec.kv_rows(i) for i in range(len(ref_cache))]
    for (layer, name), (err, bar) in llm_ref64.cache_errors(got, ref_cache).items():
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e}"


def _run_verify_sampled(dec, ref, cfg, seed):
    done = 0
    for penalty in (1.0, 1.3):
        params = dict(MAIN, repetition_penalty=penalty)
        for n_draft in (1, 3, 7):
            for a_want in sorted({0, 1, n_draft}):
                case = None
                for prompt in _distinct_prompts(seed + 10 * n_draft + a_want, ref):
                    case = S.build_block(ref, prompt[:-1], prompt[-1], n_draft, a_want, params, avoid=_eos(cfg))
                    if case:
                        break
                assert case, f"precondition: no seeded prompt gives a clear block (draft {n_draft}, accept {a_want}, penalty {penalty})"
                draft, uniforms, picks = case
                what = f"penalty {penalty} draft {n_draft} accept {a_want}"
                dec.reset()
                dec.forward(prompt[:-1], fetch=False)
                cache = ref.new()
                ref.logits(prompt[:-1], cache)
                spare = uniforms + [0.5] * (n_draft + 1 - len(uniforms))      # never used: draws_used says so
                got, a, used, logits = dec.verify_step_sampled(prompt[-1], draft, spare, history=prompt, **_sampling(params))
                assert (got, a, used) == (picks, a_want, a_want + 1), what
                want = ref.logits([prompt[-1]] + draft, list(cache))
                hist = list(prompt)
                for r in range(n_draft + 1):
                    _within(logits[r], S.penalise(want[r], hist, penalty), f"{what}: processed logits row {r}")
                    if r < n_draft:
                        hist.append(draft[r])
                ref.logits([prompt[-1]] + draft[:a], cache)
                _check_cache(dec, cache, what)
                done += 1
    assert done == 16


def test_verify_step_sampled_llama_against_float64(tmp_path):
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 3)
    _run_verify_sampled(dec, ref, cfg, 100)


def test_verify_step_sampled_head_dim_64_against_float64(tmp_path):
    dec, ref, cfg = _llama(tmp_path, HD64, 9)
    _run_verify_sampled(dec, ref, cfg, 200)


def test_verify_step_sampled_gpt2_against_float64(tmp_path):
    dec, ref, cfg = _gpt2(tmp_path)
    _run_verify_sampled(dec, ref, cfg, 300)


def test_verify_step_sampled_gguf_q8_0_q4_k_against_float64(tmp_path):
    dec, ref, cfg = _gguf(tmp_path)
    _run_verify_sampled(dec, ref, cfg, 400)


# ---- 4. the loop equals generate() and the oracle ----------------------------------------------------------------------------

N_NEW = 24


def _check_stats(st, sim):
    """The steps the host consumed are the oracle's, with its drafted and accepted counts (lookup_cases.simulate on the output)."""
    assert st["single_row_steps"] == 0
    assert st["verify_steps"] == len(sim), (st, sim)
    assert st["drafted_tokens"] == sum(m for m, _ in sim), (st, sim)
    body = sum(a for _, a in sim)
    assert st["accepted_tokens"] == body, (st, sim)


def _run_loop(dec, ref, cfg, params, seed, plan=(7, 1, 0, 2)):
    prompt, tr = _trace(ref, cfg, params, N_NEW, seed, plan=plan)
    # asserted again on what is used: the plain oracle loop on these draws gives the trace, every decision clear
    out, used, slack, clear = S.replay(ref, prompt, tr.uniforms, N_NEW, params, stops=_eos(cfg))
    assert out == tr.ids and used == N_NEW and slack >= 1.0 and clear >= 1.0
    assert tr.redraws <= S.MAX_REDRAW_RATE * N_NEW
    kw = _sampling(params)
    c0, l0 = dec.sampling_routes()
    plain, st0 = dec.generate_sampled(prompt, N_NEW, lookup=None, uniforms=tr.uniforms, **kw)
    c1, l1 = dec.sampling_routes()
    assert plain == tr.ids and st0 == dict.fromkeys(st0, 0)
    got, st = dec.generate_sampled(prompt, N_NEW, lookup=LK.DEFAULT, uniforms=tr.uniforms, **kw)
    c2, l2 = dec.sampling_routes()
    assert got == plain == tr.ids
    sim = LK.simulate(prompt, tr.ids)
    assert sim == tr.steps                                                     # the builder walked the steps the loop walks
    _check_stats(st, sim)
    assert dec.cache_len() == len(prompt) + len(got) - 1
    assert (c2 - c1) + (l2 - l1) == N_NEW == (c1 - c0) + (l1 - l0)            # one decided row per token, on either path
    return tr, (l1 - l0, l2 - l1)


def test_loop_equals_generate_and_the_oracle(tmp_path):
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4)
    tr, _ = _run_loop(dec, ref, cfg, MAIN, 1)
    full = [(m, a) for m, a in tr.steps if m and a == m]
    part = [(m, a) for m, a in tr.steps if 0 < a < m]
    none = [(m, a) for m, a in tr.steps if m and a == 0]
    assert full and part and none, tr.steps                                    # coverage: accepted, partly accepted, rejected
    # other draft lengths and n-gram bounds walk other steps to the same ids
    prompt, tr = _trace(ref, cfg, MAIN, N_NEW, 1)
    for lookup in ((1, 3, 1), (3, 2, 2), (7, 4, 1)):
        got, st = dec.generate_sampled(prompt, N_NEW, lookup=lookup, uniforms=tr.uniforms, **_sampling(MAIN))
        assert got == tr.ids, lookup
        _check_stats(st, LK.simulate(prompt, tr.ids, lookup))


@pytest.mark.parametrize("family", ["llama", "qwen2", "mistral"])
def test_loop_with_the_family_defaults(tmp_path, family):
    """Each family's default filter set (qwen2's and mistral's carry their repetition penalties), and how often a decided row
    went through the logits: at most 1 in 10, on the lookup path and on the one-row path alike."""
    params = S.FAMILY_DEFAULTS[family]
    # (logits sharpened: on the flat distributions of the unsharpened model llama's top-p 0.9 without a top-k crosses in a tail
    # of ~1e-3 masses, within the rounding of the device's sum for one row in three -- the one-row path declines those too)
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4, sharp=2.5 if family == "llama" else 2.0)
    tr, (plain_logits, lookup_logits) = _run_loop(dec, ref, cfg, params, 1)
    print(f"{family}: rows through the logits: plain {plain_logits} lookup {lookup_logits} of {N_NEW}; steps {tr.steps}")
    assert plain_logits <= N_NEW // 10, "precondition: the one-row path itself declines more than 1 row in 10 on these logits"
    assert lookup_logits <= N_NEW // 10


# ---- 5. limits -----------------------------------------------------------------------------------------------------------------

def test_limits(tmp_path):
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4)
    prompt, tr = _trace(ref, cfg, MAIN, N_NEW, 1)
    kw = _sampling(MAIN)
    starts = np.cumsum([1] + [a + 1 for _, a in tr.steps])                     # output index at which each step's row 0 is decided
    inside = [int(s) + 1 for s, (m, a) in zip(starts, tr.steps) if a >= 2]
    assert inside, "precondition: a step accepts two drafted tokens"
    # max_new_tokens reached inside an accepted draft: n_uniforms == max_new_tokens, one draw more would be refused
    for m in (0, 1, inside[0] + 1, inside[0] + 2):
        got, _ = dec.generate_sampled(prompt, m, lookup=LK.DEFAULT, uniforms=tr.uniforms[:m] if m else None, **kw)
        assert got == tr.ids[:m], m
        assert dec.generate_sampled(prompt, m, lookup=None, uniforms=tr.uniforms[:m] if m else None, **kw)[0] == got
    # a stop id sampled at row 2 of a block: nothing after it is emitted; draws used = tokens decided (the stop included)
    at = next((i for i in range(1, N_NEW) if tr.rows[i - 1] == 2 and tr.ids[i] not in tr.ids[:i]), None)
    assert at is not None, "precondition: no token first appears at row 2 of a block"
    stop = tr.ids[at]
    got, _ = dec.generate_sampled(prompt, at + 1, lookup=LK.DEFAULT, uniforms=tr.uniforms[:at + 1], stop_ids=[stop], **kw)
    assert got == tr.ids[:at]
    assert dec.cache_len() == len(prompt) + at - 1
    assert dec.generate_sampled(prompt, at + 1, lookup=None, uniforms=tr.uniforms[:at + 1], stop_ids=[stop], **kw)[0] == got
    # on_token returning false, inside a block
    seen = []
    got, _ = dec.generate_sampled(prompt, N_NEW, lookup=LK.DEFAULT, uniforms=tr.uniforms, **kw,
                                  on_token=lambda t: seen.append(t) or len(seen) < inside[0] + 1)
    assert got == seen == tr.ids[:inside[0] + 1]
    seen = []
    got, _ = dec.generate_sampled(prompt, N_NEW, lookup=LK.DEFAULT, uniforms=tr.uniforms, on_token=seen.append, **kw)
    assert got == seen == tr.ids


def test_the_end_of_the_cache(tmp_path):
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4, max_context=48)
    assert dec.context == 48
    kw = _sampling(MAIN)
    rng = np.random.default_rng(77)
    found = None
    for _ in range(8):
        a = rng.integers(4, ref.vocab, 9).tolist()
        prompt = (a * 5)[:40]                                                   # 40 of 48 rows taken; repeats, so steps draft
        try:
            found = prompt, S.build_trace(ref, prompt, 8, MAIN, avoid=_eos(cfg), plan=(7, 7, 7))
            break
        except AssertionError:
            continue
    assert found, "precondition: no seeded 40-token prompt gives a clear trace"
    prompt, tr = found
    want, used, slack, clear = S.replay(ref, prompt, tr.uniforms + [0.5] * 8, 16, MAIN, stops=_eos(cfg), context=48)
    assert want == tr.ids and used == 8 and slack >= 1.0 and clear >= 1.0       # the context ends the run, no draw past it
    for D in (7, 2):
        got, st = dec.generate_sampled(prompt, 16, lookup=(D, 3, 1), uniforms=tr.uniforms + [0.5] * 8, **kw)
        assert got == want and dec.cache_len() == 47, D
    # the last cache rows against the oracle: rows [0, 47) hold the prompt and the first seven picks
    cache = ref.new()
    ref.logits(prompt + want[:-1], cache)
    _check_cache(dec, cache, "the end of the cache")
    assert dec.generate_sampled(prompt, 16, lookup=None, uniforms=tr.uniforms + [0.5] * 8, **kw)[0] == want


# ---- 6. the fall-back, row by row --------------------------------------------------------------------------------------------

def test_rows_that_decline_fall_back_to_their_logits(tmp_path):
    """min-p 1e-4 alone keeps every token of a 320-token vocabulary: the cut hands all of them over, which the host declines
    (nothing was cut), so every decided row fetches its processed logits row -- on the lookup path as on the plain path.  The
    ids are equal and tokens_from_logits() moves by exactly the rows decided.  The everyday set right after, on the same
    handle and buffers, decides from the candidates again."""
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4)
    wide = dict(temperature=1.0, top_k=None, top_p=None, min_p=1e-4, repetition_penalty=1.0)
    n = 12
    prompt, tw = _trace(ref, cfg, wide, n, 1)
    assert any(a for _, a in tw.steps), "precondition: no step of the run accepts a drafted token"
    c0, l0 = dec.sampling_routes()
    plain, _ = dec.generate_sampled(prompt, n, lookup=None, uniforms=tw.uniforms, **_sampling(wide))
    c1, l1 = dec.sampling_routes()
    got, st = dec.generate_sampled(prompt, n, lookup=LK.DEFAULT, uniforms=tw.uniforms, **_sampling(wide))
    c2, l2 = dec.sampling_routes()
    assert got == plain == tw.ids
    assert (c1 - c0, l1 - l0) == (0, n), "precondition: the one-row path decides some of these rows from its candidates"
    assert (c2 - c1, l2 - l1) == (0, n)                                        # exactly the decided rows, none of the others
    prompt, tr = _trace(ref, cfg, MAIN, N_NEW, 1)
    got, _ = dec.generate_sampled(prompt, N_NEW, lookup=LK.DEFAULT, uniforms=tr.uniforms, **_sampling(MAIN))
    c3, l3 = dec.sampling_routes()
    assert got == tr.ids and l3 - l2 <= N_NEW // 10 and (c3 - c2) + (l3 - l2) == N_NEW


def _token_row_model(tmp_path):
    """A Llama-layout model whose logits row depends on the row's input token alone (o_proj and down_proj are zero, so the
    residual stream is the token's embedding), with an untied head bent so that four tokens have designed rows:
      Q, Y, W: three well separated leaders (0, -0.1, -0.2), everything else 3 and more below: the cut hands over 3 candidates;
      X: NEARLY FLAT -- five leaders within 0.1 of the maximum and every other token between 0.72 and 0.92 below it: under
         min-p 0.5 (threshold ln 0.5 = -0.693, the cut reaches 0.943) every token of the vocabulary is a candidate, which the
         host declines (nothing was cut) -- this row, and no other, needs its logits.
    Returns (decoder, reference, config, tokens Q Y X W)."""
    import kjarni_amd
    from safetensors.numpy import save_file
    base = dict(synth.LLAMA_TEST, tie_word_embeddings=False)
    d = str(tmp_path / "token-rows")
    cfg, t = synth.llm_model(d, base, seed=11)
    t = dict(t)
    for i in range(cfg["num_hidden_layers"]):
        for name in ("self_attn.o_proj", "mlp.down_proj"):
            t[f"model.layers.{i}.{name}.weight"] = np.zeros_like(t[f"model.layers.{i}.{name}.weight"])
    V = cfg["vocab_size"]
    Q, Y, X, W = 10, 20, 30, 40
    E, g = t["model.embed_tokens.weight"].astype(np.float64), t["model.norm.weight"].astype(np.float64)
    xs = np.stack([E[k] / np.sqrt(np.mean(E[k] ** 2) + cfg["rms_norm_eps"]) * g for k in (Q, Y, X, W)], axis=1)     # [hidden, 4]
    rng = np.random.default_rng(5)

    def leaders(first, others):
        z = -3.0 - 0.01 * rng.permutation(V).astype(np.float64)
        z[first], z[others[0]], z[others[1]] = 0.0, -0.1, -0.2
        return z
    flat = -0.72 - 0.2 * rng.permutation(V).astype(np.float64) / V
    flat[[W, 50, 60, 70, 80]] = [0.0, -0.02, -0.04, -0.06, -0.08]
    Z = np.stack([leaders(Y, (51, 52)), leaders(X, (53, 54)), flat, leaders(55, (56, 57))], axis=1)                  # [vocab, 4]
    H0 = 3.0 * t["lm_head.weight"].astype(np.float64)
    t["lm_head.weight"] = (H0 + (Z - H0 @ xs) @ np.linalg.pinv(xs)).astype(np.float32)
    save_file({k: np.ascontiguousarray(v) for k, v in t.items()}, os.path.join(d, "model.safetensors"))
    return kjarni_amd.HipDecoder(d), S.Llama64(t, cfg), cfg, (Q, Y, X, W)


def test_a_nearly_flat_middle_row_falls_back_alone(tmp_path):
    """One block whose middle row is nearly flat: rows 0 and 2 decide from their candidates, row 1 fetches its logits row --
    tokens_from_logits() moves by exactly that row -- through the hook and through the loop, whose ids equal the plain path's
    and the oracle's."""
    dec, ref, cfg, (Q, Y, X, W) = _token_row_model(tmp_path)
    params = dict(temperature=1.0, top_k=None, top_p=None, min_p=0.5, repetition_penalty=1.0)
    kw = _sampling(params)
    M = S.u_margin(1.0, 1.0)
    prompt = [Q, Y, X, W, 90, Q]                       # the history ... Q, Y drafts X, W, 90, Q: row 0 reads Y, row 1 X, row 2 W
    # the oracle's rows and the steered draws: Q -> Y, Y -> X, X -> W, W -> its leader; every precondition asserted
    want, uniforms, cache = [], [], ref.new()
    row = ref.logits(prompt, cache)[-1]
    for target in (Y, X, W, 55):
        ids, probs, slack = S.distribution(row, **params)
        u = S.steer(ids, probs, target, M)
        assert slack >= 1.0 and u is not None, f"precondition: the row in front of {target}"
        want.append(target)
        uniforms.append(u)
        row = ref.logits([target], cache)[-1]
    assert LK.lookup_draft(prompt + [Y], 3, 1, 7)[:2] == [X, W]
    # the hook: token Y, draft X, W on the prompt's cache
    dec.reset()
    dec.forward(prompt, fetch=False)
    c0, l0 = dec.sampling_routes()
    picks, a, used, logits = dec.verify_step_sampled(Y, [X, W], uniforms[1:], **kw)
    c1, l1 = dec.sampling_routes()
    assert (picks, a, used) == (want[1:], 2, 3)
    assert (c1 - c0, l1 - l0) == (2, 1)                                        # rows 0 and 2 from candidates, row 1 from its logits
    spread = np.sort(logits[1])[::-1]
    assert spread[0] - spread[-1] < 0.943 and spread[0] - spread[5] > 0.7      # the flat row is the one the test built
    # the loop: the first token from the prompt's row, then one block of which the middle row falls back
    plain, _ = dec.generate_sampled(prompt, 4, lookup=None, uniforms=uniforms, **kw)
    c2, l2 = dec.sampling_routes()
    got, st = dec.generate_sampled(prompt, 4, lookup=LK.DEFAULT, uniforms=uniforms, **kw)
    c3, l3 = dec.sampling_routes()
    assert got == plain == want
    assert (st["verify_steps"], st["accepted_tokens"]) == (1, 2)
    assert (c3 - c2, l3 - l2) == (3, 1)                                        # 4 rows decided, exactly one through the logits
    assert l2 - l1 >= 1                                                        # (the plain path needed that row's logits too)


# ---- 7. the Generator ----------------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "1 2 3 4 5 6 7 8 9 1 2 3 4 5", "Once upon a time there was a small"]


def test_generator_prompt_lookup_sampling(tmp_path):
    from kjarni_amd import BpeTokenizer, Generator
    from kjarni_amd.chat import GenerationConfig
    from tests.gpt2_ref64 import Gpt2Ref64
    d = str(tmp_path / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen = Generator("gpt2", model_path=d)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    ref = Gpt2Ref64(t, cfg)
    want = ["".join(tok.decode([i], skip_special=False) for i in ref.greedy(gen.encode(text), 30, stop=(G.ENDOFTEXT,))) for text in TEXTS]
    k1 = GenerationConfig(do_sample=True, top_k=1, max_new_tokens=30)          # sampling that can only take the best token
    k50 = GenerationConfig(do_sample=True, top_k=50, max_new_tokens=20)
    pen = GenerationConfig(do_sample=True, top_k=50, max_new_tokens=20, repetition_penalty=1.3)
    # the setter off (the default): sampled and penalty configs stay on the plain path, whatever set_prompt_lookup says
    gen.set_prompt_lookup(7)
    gen.seed(11)
    plain = [gen.generate(text, c) for text in TEXTS for c in (k1, k50, pen)]
    assert gen.verify_gemv_calls() == (0, 0)
    assert plain[0::3] == want                                                  # top_k = 1 is the greedy text
    # on: the same seed gives the same texts through the lookup loop
    gen.set_prompt_lookup_sampling(True)
    gen.seed(11)
    assert [gen.generate(text, c) for text in TEXTS for c in (k1, k50, pen)] == plain
    moved = gen.verify_gemv_calls()
    assert sum(moved) > 0
    # draw accounting: after a lookup-sampled call the generator's stream is where the plain call leaves it
    gen.seed(5)
    gen.generate(TEXTS[1], k50)
    b_after_lookup = gen.generate(TEXTS[0], k50)
    gen.set_prompt_lookup_sampling(False)
    gen.seed(5)
    before = gen.verify_gemv_calls()
    gen.generate(TEXTS[1], k50)
    assert gen.generate(TEXTS[0], k50) == b_after_lookup and gen.verify_gemv_calls() == before
    # off again, and without set_prompt_lookup: nothing moves
    gen.set_prompt_lookup_sampling(True)
    gen.set_prompt_lookup(0)
    gen.seed(11)
    assert [gen.generate(text, c) for text in TEXTS for c in (k1, k50, pen)] == plain and gen.verify_gemv_calls() == before


def test_requests_the_sampled_loop_does_not_take(tmp_path):
    """The stated forwarding outcomes of the sampled entry: lookup = None is the plain loop (stats zero); greedy with a penalty
    and any n-gram ban forward to it as well (stats zero, no verify step); greedy without processors takes the greedy lookup
    loop.  (The greedy entry generate_lookup has no way to ask for sampling: its own contract is tests/test_gpu_lookup.py's.)"""
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4)
    prompt = next(_prompts(1, ref))
    u = [0.5] * 8
    zero = dict(verify_steps=0, drafted_tokens=0, accepted_tokens=0, single_row_steps=0)
    assert dec.generate_sampled(prompt, 8, lookup=None, uniforms=u, **_sampling(MAIN))[1] == zero
    for kw in (dict(sample=False, repetition_penalty=1.3), dict(no_repeat_ngram=2, **_sampling(MAIN)), dict(sample=False, no_repeat_ngram=2)):
        before = dec.verify_gemv_calls()
        got, st = dec.generate_sampled(prompt, 8, lookup=LK.DEFAULT, uniforms=u, **kw)
        assert st == zero and dec.verify_gemv_calls() == before, kw
        assert got == dec.generate_sampled(prompt, 8, lookup=None, uniforms=u, **kw)[0]
    got, st = dec.generate_sampled(prompt, 8, lookup=LK.DEFAULT, sample=False)      # greedy without processors: the greedy lookup loop
    assert got == dec.generate(prompt, 8) and st["verify_steps"] >= 1


# ---- 8. errors before any GPU work ---------------------------------------------------------------------------------------------

def test_errors(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    dec, ref, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4, max_context=48)
    kw = _sampling(MAIN)
    seen = []
    for lookup, field in (((0, 3, 1), "draft_tokens"), ((8, 3, 1), "draft_tokens"), ((7, 5, 1), "ngram_max"), ((7, 0, 1), "ngram_max"),
                          ((7, 3, 0), "ngram_min"), ((7, 2, 3), "ngram_min")):
        with pytest.raises(KjarniException, match=field) as e:
            dec.generate_sampled([5, 6, 7], 4, lookup=lookup, uniforms=[0.5] * 4, on_token=seen.append, **kw)
        assert e.value.code == E.INVALID_CONFIG and seen == []
    with pytest.raises(KjarniException, match="context") as e:
        dec.generate_sampled(list(range(4, 4 + 49)), 4, lookup=LK.DEFAULT, uniforms=[0.5] * 4, on_token=seen.append, **kw)
    assert e.value.code == E.INVALID_CONFIG and seen == []
    with pytest.raises(KjarniException, match="empty prompt") as e:
        dec.generate_sampled([], 4, lookup=LK.DEFAULT, uniforms=[0.5] * 4, **kw)
    assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(KjarniException, match="n_uniforms") as e:
        dec.generate_sampled([5, 6, 7], 4, lookup=LK.DEFAULT, uniforms=[0.5] * 3, **kw)
    assert e.value.code == E.INVALID_CONFIG
    dec.reset()
    dec.forward(list(range(4, 4 + 42)), fetch=False)
    for draft, rows in (([5, 6, 7], 3), ([5, 6, 7], 9), ([5], 0)):
        with pytest.raises(KjarniException, match="rows") as e:
            dec.verify_step_sampled(4, draft, [0.5] * 8, rows=rows, **kw)
        assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(KjarniException, match="context") as e:                 # 42 + 7 rows > 48
        dec.verify_step_sampled(4, [5, 6], [0.5] * 8, rows=7, **kw)
    assert e.value.code == E.INVALID_CONFIG and dec.cache_len() == 42
    picks, a, used, _ = dec.verify_step_sampled(4, [5, 6], [0.5] * 8, rows=6, **kw)   # 42 + 6 rows == 48 fits
    assert len(picks) == a + 1 == used and dec.cache_len() == 42 + a + 1
