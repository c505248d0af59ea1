"""Constrained decoding on the GPU: the three kernels alone (kjarni_hip_op_constraint_*) against numpy, then the loops of
kjarni_hip_decoder_generate_constrained on a tiny Llama against the float64 oracle of tests/constraint_cases.py (the mask applied
in Python), the properties that hold whatever the logits, the universal pattern against the plain loops, every way a run ends,
the refusals, and the Generator and Chat end to end on a fixture tokenizer."""
import os
import re
import shutil

import numpy as np
import pytest

from tests import constraint_cases as CC
from tests import gpt2_fixture as G
from tests import sampled_lookup_cases as SC
from tests import synth

pytestmark = pytest.mark.gpu
CAP = 40
STOPS = [2, 3]                                                    # LLAMA_TEST's eos ids
SAMPLED = dict(temperature=0.8, top_k=12, top_p=None, min_p=0.02)
PENALTY = 1.3
LOOPS = ("greedy", "penalty", "penalty-host", "sampled", "sampled-host")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _K():
    from kjarni_amd import constraints
    return constraints


# ---- the mask build alone ---------------------------------------------------------------------------------------------------------

def _mask_tokens(V, seed):
    """Tokens of 0, 1 and 40 bytes, one that dies on its last byte, one that passes through an accepting state into a
    non-accepting one (for the pattern (?:ab)*c?), and seeded strings over the pattern's alphabet."""
    rng = np.random.default_rng(seed)
    fixed = [b"", b"a", b"ab" * 20, b"ababx", b"aba", b"c", b"abc", b"b", b"", b"abab"]
    out = []
    for i in range(V):
        if i < len(fixed):
            out.append(fixed[i])
        else:
            out.append(bytes(rng.choice(list(b"abc"), int(rng.integers(0, 7))).tolist()))
    out[V - 1] = b"ab"                                           # the last token of the last (partial) word is allowed from the start
    return out


def _check_mask(trans, tokens):
    from kjarni_amd import ops
    off, data = CC.table(tokens)
    mask, counts = ops.constraint_mask(trans, off, data)
    want = CC.allowed_matrix(trans, tokens)
    V = len(tokens)
    assert (mask == CC.pack(want)).all()
    bits = CC.unpack(mask, V)
    assert not bits[:, V:].any(), "bits at or past the vocabulary are set"
    assert (bits[:, :V] == want).all()
    assert (counts == want.sum(axis=1)).all()
    return want


@pytest.mark.parametrize("V", [257, 300, 4097])
@pytest.mark.parametrize("pattern,S", [(r"", 1), (r"a", 2), (r"(?:ab)*c?", 3), (r"[ab]{0,63}c", 65)])
def test_mask_build_matches_a_numpy_walk(V, pattern, S):
    r = _K().Regex(pattern)
    assert r.states == S
    tokens = _mask_tokens(V, V + S)
    want = _check_mask(r.trans, tokens)
    if pattern == r"(?:ab)*c?":
        q_ab = CC.walk(r.trans, 0, b"ab")
        assert r.accepting[0] and r.accepting[q_ab] and not r.accepting[CC.walk(r.trans, 0, b"a")]
        assert not want[0, 0] and not want[0, 8]                  # no bytes: never allowed
        assert want[0, 1] and want[0, 2]                          # 1 byte, 40 bytes
        assert not want[0, 3] and CC.walk(r.trans, 0, b"abab") != CC.DEAD   # dies on its last byte
        assert want[0, 4]                                         # through an accepting state into a non-accepting one
        assert want[0, V - 1]


@pytest.mark.parametrize("V", [128256, 151936])
def test_mask_build_at_production_vocabularies(V):
    K = _K()
    r = K.Regex(K.json_object({"id": K.integer(), "ok": K.choices(["true", "false"])}))
    assert 15 <= r.states <= 40
    rng = np.random.default_rng(V)
    alphabet = np.frombuffer(b"{}\":,idoktruefals0123456789- ", np.uint8)
    lens = rng.integers(0, 9, V)
    lens[7], lens[V - 1] = 40, 1
    flat = alphabet[rng.integers(0, alphabet.size, int(lens.sum()))]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    tokens = [flat[cuts[i]:cuts[i + 1]].tobytes() for i in range(V)]
    tokens[3], tokens[V - 1] = b"{\"id\":", b"{"
    want = _check_mask(r.trans, tokens)
    assert want[0, 3] and want[0, V - 1] and want.sum() > r.states


# ---- apply and advance alone ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """(?:yes|no)!? over a 300-token table; 7 = "yes", 8 = "no", 9 = "!", 5 = a stop id without bytes, 10 = a stop id with bytes."""
    K = _K()
    tokens = CC.model_tokens(300, specials=(0, 1, 2, 3, 5))
    tokens[7], tokens[8], tokens[9], tokens[10], tokens[11], tokens[12] = b"yes", b"no", b"!", b"y", b"es", b"ye"
    con = K.Constraint(r"(?:yes|no)!?", tokens)
    return con, CC.HostConstraint(con.regex, tokens, [5, 10])


@pytest.mark.parametrize("rows", [1, 3])
def test_apply_keeps_allowed_logits_bit_for_bit(small, rows):
    from kjarni_amd import ops
    con, hc = small
    V, ld = con.vocab, con.vocab + 9
    rng = np.random.default_rng(rows)
    logits = rng.standard_normal((rows, ld)).astype(np.float32)
    logits[:, V:] = np.nan                                        # canaries behind every row (and so in front of the next)
    logits[0, 7] = np.float32(-0.0)
    q_yes = hc.step(hc.start, 7)                                  # accepting, not closed
    q_y = hc.step(hc.start, 10)                                   # not accepting
    states = [hc.start, q_yes, q_y][:rows]
    done = [0] * rows
    out = ops.constraint_apply(con, logits, states, done, stop_ids=hc.stops)
    for r_, q in enumerate(states):
        legal = hc.legal(q)
        assert (out[r_, :V][legal].view(np.uint32) == logits[r_, :V][legal].view(np.uint32)).all()
        assert np.isneginf(out[r_, :V][~legal]).all()
        assert np.isnan(out[r_, V:]).all() and (out[r_, V:].view(np.uint32) == logits[r_, V:].view(np.uint32)).all()
        # a stop id is governed by the accepting rule alone: 10 ("y") has bytes that pass the mask at the start, and is masked there
        assert bool(legal[5]) == bool(legal[10]) == bool(hc.accepting[q])
    assert hc.allowed[hc.start, 10] and np.isneginf(out[0, 10]) and np.isneginf(out[0, 5])
    if rows == 3:
        assert np.isfinite(out[1, 5]) and np.isfinite(out[1, 10]) and np.isfinite(out[1, 9])
        # a row whose done flag is set is left untouched
        out2 = ops.constraint_apply(con, logits, states, [0, 1, 0], stop_ids=hc.stops)
        assert (out2[1].view(np.uint32) == logits[1].view(np.uint32)).all()
        assert (out2[[0, 2]].view(np.uint32) == out[[0, 2]].view(np.uint32)).all()
    # without stop ids in the call nothing but the mask decides
    out3 = ops.constraint_apply(con, logits, states, done)
    assert (np.isfinite(out3[0, :V]) == hc.allowed[states[0]]).all()


def test_advance_every_branch(small):
    from kjarni_amd import ops
    con, hc = small
    q0, q_yes, q_y = hc.start, hc.step(hc.start, 7), hc.step(hc.start, 10)
    q_end = hc.step(q_yes, 9)
    assert hc.closed[q_end] and hc.accepting[q_yes] and not hc.closed[q_yes]
    cases = [  # (state, done, pick) -> (state, done, violated)
        ((q0, 0, 7), (q_yes, 0, 0)),         # an allowed token walks its bytes
        ((q0, 0, 12), (hc.step(q0, 12), 0, 0)),
        ((q_yes, 0, 9), (q_end, 1, 0)),      # into a closed state: done
        ((q_yes, 0, 5), (q_yes, 1, 0)),      # a stop id in an accepting state keeps the state and sets done
        ((q_yes, 0, 10), (q_yes, 1, 0)),     # ... a stop id that has bytes too
        ((q0, 0, 5), (q0, 1, 1)),            # a stop id outside an accepting state: violated
        ((q0, 0, 9), (q0, 1, 1)),            # a token whose walk dies: violated, the state kept
        ((q0, 0, 0), (q0, 1, 1)),            # a token without bytes
        ((q0, 0, -1), (q0, 1, 1)),           # no token at all
        ((q0, 0, 100000), (q0, 1, 1)),       # past the vocabulary
        ((q_y, 1, 11), (q_y, 1, 0)),         # done: the state no longer moves
        ((q_y, 0, 11), (q_yes, 0, 0)),
    ]
    st, dn, bad = ops.constraint_advance(con, [c[0][2] for c in cases], [c[0][0] for c in cases], [c[0][1] for c in cases], stop_ids=hc.stops)
    got = list(zip(st.tolist(), dn.tolist(), bad.tolist()))
    assert got == [c[1] for c in cases]
    # violated stays 0 on every token the mask allows, from every state; one row at a time as well
    for q in range(con.states):
        legal = np.flatnonzero(hc.legal(q))
        if not legal.size:                                       # (a state no token of this table leads on from)
            continue
        st, dn, bad = ops.constraint_advance(con, legal, [q] * legal.size, [0] * legal.size, stop_ids=hc.stops)
        assert not bad.any()
        for t, s2, d2 in zip(legal.tolist(), st.tolist(), dn.tolist()):
            if t in hc.stops:
                assert (s2, d2) == (q, 1)
            else:
                assert s2 == hc.step(q, t) and d2 == int(hc.closed[s2])
    st, dn, bad = ops.constraint_advance(con, [7], [q0], [0], stop_ids=hc.stops)
    assert (st[0], dn[0], bad[0]) == (q_yes, 0, 0)


def test_device_constraint_object(small):
    con, hc = small
    want = CC.pack(hc.allowed)
    for q in range(con.states):
        assert (con.mask(q) == want[q]).all()
    assert (con.counts() == hc.allowed.sum(axis=1)).all()
    assert (con.states, con.vocab, con.words) == (hc.trans.shape[0], 300, 5)
    import kjarni_amd
    with pytest.raises(kjarni_amd.KjarniException):
        con.mask(con.states)
    # a mask beyond 256 MiB is refused before any GPU work: 4096 states x 600 000 tokens
    big = _K().Regex(r"[ab]*a[ab]{11}")
    with pytest.raises(kjarni_amd.KjarniException) as e:
        _K().Constraint(big, [b"a"] * 600000)
    assert "256" in str(e.value) or "268435456" in str(e.value)


# ---- the loops against the float64 oracle -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    import kjarni_amd
    d = str(tmp_path_factory.mktemp("constraint") / "m")
    cfg, t = synth.llm_model(d, synth.LLAMA_TEST, seed=4)
    return kjarni_amd.HipDecoder(d, max_context=CAP), SC.Llama64(t, cfg), cfg


@pytest.fixture(scope="module")
def tokens(model):
    return CC.model_tokens(model[2]["vocab_size"])


_CONS = {}


def _constraint(pattern, tokens, stops=STOPS):
    key = (pattern, id(tokens))
    if key not in _CONS:
        con = _K().Constraint(pattern, tokens)
        _CONS[key] = con
    return _CONS[key], CC.HostConstraint(_CONS[key].regex, tokens, stops)


def _prompt(seed, n=6):
    return np.random.default_rng(seed).integers(4, synth.LLAMA_TEST["vocab_size"], n).tolist()


def _run(dec, con, loop, prompt, max_new, uniforms=None, stop_ids=None, on_token=None):
    dec.set_device_sampling(not loop.endswith("-host"))
    try:
        if loop.startswith("sampled"):
            return dec.generate_constrained(con, prompt, max_new, sample=True, uniforms=uniforms if max_new else None, stop_ids=stop_ids,
                                            on_token=on_token, **SAMPLED)
        return dec.generate_constrained(con, prompt, max_new, sample=False, repetition_penalty=1.0 if loop == "greedy" else PENALTY,
                                        stop_ids=stop_ids, on_token=on_token)
    finally:
        dec.set_device_sampling(True)


def _oracle(ref, hc, loop, prompt, max_new, uniforms=None, seed=0):
    if loop.startswith("sampled"):
        return CC.oracle_run(ref, prompt, max_new, hc, params=SAMPLED, uniforms=uniforms, seed=seed, context=CAP)
    return CC.oracle_run(ref, prompt, max_new, hc, penalty=1.0 if loop == "greedy" else PENALTY, context=CAP)


def _clear_case(ref, hc, loop, max_new, seeds=range(1, 40)):
    """The first seeded prompt whose oracle run clears the float bar at every decision (near-ties are no fair demand of f32)."""
    for seed in seeds:
        prompt = _prompt(seed)
        ids, info = _oracle(ref, hc, loop, prompt, max_new, seed=seed)
        if info["clear"] and ids:
            return prompt, ids, info
    raise AssertionError("precondition: no seeded prompt clears the float bar")


PATTERNS = [r"[a-e]+(?:, [a-e]+)*\.", r"-?(?:0|[1-9][0-9]*)(?:\.[0-9]+)?", r"(?:yes|no|maybe)"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_five_loops_agree_with_the_float64_oracle(model, tokens, pattern):
    dec, ref, _ = model
    con, hc = _constraint(pattern, tokens)
    n_new = 10
    got = {}
    for loop in LOOPS:
        base = "sampled" if loop.startswith("sampled") else loop.replace("-host", "")
        if base not in got:
            prompt, want, info = _clear_case(ref, hc, base, n_new)
            got[base] = (prompt, want, info)
        prompt, want, info = got[base]
        ids, res = _run(dec, con, loop, prompt, n_new, uniforms=np.asarray(info["uniforms"] + [0.5] * n_new, np.float32)[:n_new])
        assert ids == want, (loop, pattern)
        assert res["violated"] == 0 and res["final_state"] == info["final_state"] == res["device_state"], loop
        assert res["complete"] == int(info["complete"]) and res["accepted"] == int(info["accepted"]), loop
        assert dec.resident() == (prompt + ids)[:dec.cache_len()], loop


# ---- properties that hold whatever the logits -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("loop", LOOPS)
def test_emitted_bytes_are_always_a_live_prefix(model, tokens, loop):
    dec, _, _ = model
    K = _K()
    patterns = [K.choices(["yes", "no", "maybe", "abc"]), K.integer(), K.number(), K.json_object({"a": K.integer(), "b": K.choices(["yes", "no"])}),
                r"[a-e]+(?:, [a-e]+)*\."]
    for i, pattern in enumerate(patterns):
        con, hc = _constraint(pattern, tokens)
        for seed in (1, 2):
            prompt = _prompt(10 * i + seed)
            u = np.random.default_rng(seed).random(24).astype(np.float32)
            ids, res = _run(dec, con, loop, prompt, 24, uniforms=u)
            text = hc.text(ids)
            assert not res["violated"] and hc.live_prefix(ids), (pattern, text)
            assert res["final_state"] == CC.walk(hc.trans, hc.start, text) == res["device_state"]
            assert res["accepted"] == int(hc.accepting[res["final_state"]])
            if res["complete"] or res["accepted"]:
                assert re.fullmatch(pattern, text.decode(), re.ASCII), (pattern, text)
            if res["complete"]:
                assert res["accepted"]
            if i == 0:                                           # a choices pattern ends closed after exactly one of the choices
                assert res["complete"] and hc.closed[res["final_state"]] and text in (b"yes", b"no", b"maybe", b"abc")
            assert all(t not in STOPS for t in ids)


# ---- the universal pattern: nothing but the stop rule is masked ------------------------------------------------------------------------

@pytest.mark.parametrize("loop", LOOPS)
def test_universal_pattern_equals_the_plain_loops(model, loop):
    dec, _, cfg = model
    toks = _UNIVERSAL.setdefault("t", CC.universal_tokens(cfg["vocab_size"], 2))
    con, hc = _constraint(r"(?:.|\n)*", toks, stops=[2])
    assert hc.allowed[hc.start].sum() == cfg["vocab_size"] - 1   # (the other states sit inside a multi-byte character)
    for seed, n_new in ((1, 9), (2, 20)):
        prompt = _prompt(seed)
        u = np.random.default_rng(seed).random(n_new).astype(np.float32)
        dec.set_device_sampling(not loop.endswith("-host"))
        if loop.startswith("sampled"):
            plain, _ = dec.generate_sampled(prompt, n_new, sample=True, uniforms=u, stop_ids=[2], **SAMPLED)
        else:
            plain, _ = dec.generate_sampled(prompt, n_new, sample=False, repetition_penalty=1.0 if loop == "greedy" else PENALTY, stop_ids=[2])
        dec.set_device_sampling(True)
        plain_len, plain_res = dec.cache_len(), dec.resident()
        ids, res = _run(dec, con, loop, prompt, n_new, uniforms=u, stop_ids=[2])
        assert ids == plain and dec.cache_len() == plain_len and dec.resident() == plain_res, loop
        assert res["violated"] == 0 and res["accepted"] == 1


_UNIVERSAL = {}


# ---- endings and state ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loop", LOOPS)
def test_endings(model, tokens, loop):
    dec, ref, _ = model
    base = "sampled" if loop.startswith("sampled") else loop.replace("-host", "")
    # (a) a closed state in the middle of a burst: the run ends without a stop token, what the device ran past it is discarded
    # (no token holds a whole match: the first token never closes the pattern)
    con, hc = _constraint(r"(?:yes|no|maybe)\.", tokens)
    prompt, want, info = _clear_case(ref, hc, base, 12)
    u = np.asarray(info["uniforms"] + [0.5] * 12, np.float32)[:12]
    ids, res = _run(dec, con, loop, prompt, 12, uniforms=u)
    assert ids == want and 2 <= len(ids) <= 6 and res["complete"] and res["accepted"] and hc.closed[res["final_state"]]
    assert res["device_state"] == res["final_state"]
    assert dec.resident() == (prompt + ids)[:dec.cache_len()]
    if loop == "greedy":
        assert dec.cache_len() == len(prompt) + 11               # the first burst ran to its end behind the closed state
    else:
        assert dec.cache_len() == len(prompt) + len(ids) - 1     # nothing follows the token that closed the pattern
    # (b) a stop id in an accepting state: no token has a "q", so behind a whole word the state is accepting, not closed, and
    # offers nothing but the call's stop ids -- which the accepting rule makes legal there and nowhere before
    con, hc = _constraint(r"(?:yes|no|maybe)q?", tokens)
    prompt, want, info = _clear_case(ref, hc, base, 12)
    ids, res = _run(dec, con, loop, prompt, 12, uniforms=np.asarray(info["uniforms"] + [0.5] * 12, np.float32)[:12])
    assert ids == want and info["complete"] and res["complete"] and res["accepted"] and not hc.closed[res["final_state"]]
    assert hc.text(ids) in (b"yes", b"no", b"maybe")
    assert res["device_state"] == res["final_state"] == CC.walk(hc.trans, hc.start, hc.text(ids))
    assert dec.resident() == (prompt + ids)[:dec.cache_len()]
    if loop != "greedy":
        assert dec.cache_len() == len(prompt) + len(ids)          # every emitted token was fed: the stop id came from the last one
    # (c) max_new_tokens in a state that is not accepting
    con, hc = _constraint(r"[a-e]{30}\.", tokens)
    prompt = _prompt(5)
    u = np.random.default_rng(5).random(6).astype(np.float32)
    ids, res = _run(dec, con, loop, prompt, 6, uniforms=u)
    assert len(ids) == 6 and res["accepted"] == 0 and res["complete"] == 0 and res["violated"] == 0
    assert res["final_state"] == CC.walk(hc.trans, hc.start, hc.text(ids)) == res["device_state"]
    assert dec.cache_len() == len(prompt) + 5 and dec.resident() == (prompt + ids)[:-1]
    ids0, res0 = _run(dec, con, loop, prompt, 0)
    assert ids0 == [] and res0["final_state"] == hc.start and res0["accepted"] == 0 and dec.cache_len() == len(prompt)
    # (d) the callback stops the run at token 2
    seen = []
    ids2, res2 = _run(dec, con, loop, prompt, 6, uniforms=u, on_token=lambda t: seen.append(t) or len(seen) < 2)
    assert ids2 == seen == ids[:2] and res2["complete"] == 0
    assert res2["final_state"] == CC.walk(hc.trans, hc.start, hc.text(ids2)) == res2["device_state"]
    assert dec.resident() == (prompt + ids2)[:dec.cache_len()]
    assert dec.cache_len() == len(prompt) + (4 if loop == "greedy" else 1)
    # (e) the capacity
    long_prompt = _prompt(6, CAP - 4)
    ids3, res3 = _run(dec, con, loop, long_prompt, 10, uniforms=np.random.default_rng(6).random(10).astype(np.float32))
    assert len(ids3) == 4 and res3["accepted"] == 0 and hc.live_prefix(ids3)
    assert res3["final_state"] == CC.walk(hc.trans, hc.start, hc.text(ids3)) == res3["device_state"]
    assert dec.cache_len() == (CAP if loop == "greedy" else CAP - 1) and dec.resident() == (long_prompt + ids3)[:dec.cache_len()]


# ---- refusals and surface --------------------------------------------------------------------------------------------------------------

def test_refusals_before_any_gpu_work(model, tokens):
    import kjarni_amd
    dec, _, cfg = model
    dec.generate(_prompt(1), 3)
    before = (dec.cache_len(), dec.resident())
    K = _K()
    # "x" is no token and no prefix of one: from the start state nothing can be emitted
    toks = [b"" if i < 4 else b"a" for i in range(cfg["vocab_size"])]
    stuck = K.Constraint(r"ax", toks)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_constrained(stuck, _prompt(1), 4)
    assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and "state 1" in str(e.value)
    # accepting but not closed, and the only way on is a stop id with bytes: subtracted, so refused without ... and fine with stop ids
    toks2 = list(toks)
    toks2[9] = b"b"
    loose = K.Constraint(r"a+b?", toks2)
    ids, res = dec.generate_constrained(loose, _prompt(1), 3, stop_ids=[2])
    assert len(ids) <= 3 and res["violated"] == 0
    only_stop = K.Constraint(r"b*", toks2)                        # the start state allows token 9 alone, and 9 is the call's stop id
    ids, res = dec.generate_constrained(only_stop, _prompt(1), 3, stop_ids=[9])
    assert ids == [] and res["complete"] == 1                     # accepting: the stop id is legal at once
    no_way = K.Constraint(r"b+", toks2)                           # ... not accepting: nothing but the stop id could be emitted
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_constrained(no_way, _prompt(1), 3, stop_ids=[9])
    assert "state 0" in str(e.value)
    # another vocabulary, too many stop ids
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_constrained(K.Constraint(r"a+", toks[:100]), _prompt(1), 3)
    assert "100" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_constrained(stuck, _prompt(1), 3, stop_ids=list(range(100, 117)))
    assert "16" in str(e.value)
    dec.generate(_prompt(1), 0)
    assert before[1][:6] == dec.resident()[:6]                    # (the refused calls ran nothing: the model still answers)


def test_generator_and_chat_end_to_end(tmp_path):
    from kjarni_amd import BpeTokenizer, Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    K = _K()
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    gen = Generator("gpt2", model_path=d)
    greedy = GenerationConfig(do_sample=False, max_new_tokens=24)
    prompt = "The quick brown fox"
    plain = gen.generate(prompt, greedy)
    pattern = K.json_object({"answer": K.choices(["yes", "no"]), "n": K.integer()})
    gen.set_constraint(pattern)
    gen.set_prompt_lookup(4)                                      # a constrained request takes the plain loop all the same
    for config in (greedy, GenerationConfig(temperature=1.3, max_new_tokens=24), GenerationConfig(do_sample=False, max_new_tokens=24,
                                                                                                 repetition_penalty=1.2)):
        gen.seed(7)
        text = gen.generate(prompt, config)
        res = gen.constraint_result()
        assert res["violated"] == 0
        full = K.Regex(pattern)
        assert full.step(full.start, text.encode()) != CC.DEAD, text
        if res["complete"]:
            assert re.fullmatch(pattern, text, re.ASCII), text
    gen.set_constraint(K.choices(["yes", "no", " maybe"]))
    assert gen.generate(prompt, greedy) in ("yes", "no", " maybe") and gen.constraint_result()["complete"] == 1
    pieces = []
    gen.stream(prompt, lambda s: pieces.append(s) or True, greedy)
    assert "".join(pieces) in ("yes", "no", " maybe")
    import kjarni_amd
    with pytest.raises(kjarni_amd.KjarniException):
        gen.set_constraint("a*?")
    assert gen.generate(prompt, greedy) in ("yes", "no", " maybe")  # a refused pattern leaves the old one in place
    gen.set_prompt_lookup(0)
    gen.set_constraint(None)
    assert gen.generate(prompt, greedy) == plain                  # None restores the plain behaviour exactly
    assert b"".join(tok.token_bytes(i) for i in tok.encode(" maybe")) == b" maybe"
    gen.close()

    ld = str(tmp_path / "llama")
    synth.llm_model(ld, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(ld, "tokenizer.json"))
    chat = Chat("llama3.2-1b-instruct", model_path=ld)
    cfg = GenerationConfig(do_sample=False, max_new_tokens=16)
    plain = chat.send("Is water wet?", cfg)
    chat.set_constraint(K.choices(["Yes.", "No."]))
    assert chat.send("Is water wet?", cfg) in ("Yes.", "No.")
    assert chat.constraint_result()["complete"] == 1 and chat.constraint_result()["violated"] == 0
    chat.set_constraint(None)
    assert chat.send("Is water wet?", cfg) == plain
