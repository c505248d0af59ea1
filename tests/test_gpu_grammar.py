"""Grammar-constrained decoding on the GPU: the two kernels alone (kjarni_hip_op_grammar_*) bit for bit against the table walker of
tests/grammar_cases.py, then the loops of kjarni_hip_decoder_generate_grammar on the tiny Llama and GPT-2 fixtures against the
float64 oracle of tests/constraint_cases.py driven by HostGrammar, the properties that hold whatever the logits, every way a run
ends, the refusals, and the Generator and Chat end to end on fixture tokenizers."""
import json
import os
import shutil

import numpy as np
import pytest

from tests import constraint_cases as CC
from tests import gpt2_fixture as G
from tests import grammar_cases as GC
from tests import sampled_lookup_cases as SC
from tests import synth

pytestmark = pytest.mark.gpu
CAP = 112
SAMPLED = dict(temperature=0.8, top_k=12, top_p=None, min_p=0.02)
PENALTY = 1.3
LOOPS = ("greedy", "penalty", "penalty-host", "sampled", "sampled-host")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAN = np.float32(np.nan)


def _K():
    from kjarni_amd import constraints
    return constraints


# ---- apply alone ------------------------------------------------------------------------------------------------------------------------

FIXED = [b"", b"}", b"}}", b"\"}]", b"[]", b"{\"a\":[", b"[" * 8, b"[" * 8 + b"1", b"", b"\xc3", b"\xa9", b"\xc3\xa9", b"\"", b"1", b",", b"]", b"[", b"{",
         b":", b"\"a\"", b"]]]", b",[", b"1]", b"true", b"nul", b"\"\xe2\x82", b"\xac\"", b"[[", b"]],", b" ", b"e", b"-", b"0", b"\\", b"\\n"]


def _vocabulary(V, seed):
    """The fixed tokens above (pops of one, two and three levels, pushes and pops inside one token, 16 and 17 own pushes, empty
    tokens, a two-byte and a three-byte character whole and split), then seeded strings over JSON's alphabet; the first and the
    last id have bytes of their own and double as stop ids."""
    rng = np.random.default_rng(seed)
    alphabet = b"{}[]\",:01a"
    out = [b"1"] + FIXED
    while len(out) < V:
        out.append(bytes(alphabet[int(j)] for j in rng.integers(0, len(alphabet), int(rng.integers(0, 4)))))
    out = out[:V]
    out[V - 1] = b"]"
    return out


@pytest.fixture(scope="module")
def jv():
    K = _K()
    g = K.Grammar(K.json_value())
    walked = {name: GC.walk(g.action, g.flags, GC.START, data) for name, data in
              dict(start=b"", one=b"1", in_array=b"[", closed=b"[]", d63=b"[" * 32, d64=b"[" * 32 + b"1", d64s=b"[" * 32 + b"\"", obj=b"{\"a\":[1,{\"b\":",
                   after_key=b"{\"a\"", mid_char=b"[\"\xc3", three=b"[[{\"a\":\"x").items()}
    assert None not in walked.values()
    assert [len(walked[k][1]) for k in ("start", "one", "in_array", "d63", "d64", "d64s")] == [0, 0, 1, 63, 64, 64]
    assert GC.accepted(g.flags, walked["one"]) and GC.accepted(g.flags, walked["closed"]) and GC.closed(g.flags, walked["closed"])
    assert not GC.accepted(g.flags, walked["start"]) and not GC.accepted(g.flags, walked["in_array"])
    # the tokens of 16 and 17 own pushes, from inside an array (a value and an array per bracket, one more value for the digit)
    assert GC.own_pushes_peak(g.action, g.flags, walked["in_array"], b"[" * 8) == 16
    assert GC.own_pushes_peak(g.action, g.flags, walked["in_array"], b"[" * 8 + b"1") == 17
    assert GC.walk(g.action, g.flags, walked["in_array"], b"[" * 8, True) is not None
    assert GC.walk(g.action, g.flags, walked["in_array"], b"[" * 8 + b"1", True) is None
    assert GC.walk(g.action, g.flags, walked["in_array"], b"[" * 8 + b"1", False) is not None
    return g, walked


_CONS = {}


def _device_grammar(g, V):
    if V not in _CONS:
        tokens = _vocabulary(V, V)
        _CONS[V] = (_K().GrammarConstraint(g, tokens), tokens)
    return _CONS[V]


def _reference(g, tokens, logits, configs, done, stops):
    """apply_reference with the walks memoised by the token's bytes (the large vocabularies repeat short strings)."""
    out = logits.copy()
    for r, c in enumerate(configs):
        if done[r]:
            continue
        memo = {}
        ok_stop = GC.accepted(g.flags, c)
        for t, data in enumerate(tokens):
            if t in stops:
                ok = ok_stop
            else:
                if data not in memo:
                    memo[data] = len(data) > 0 and GC.walk(g.action, g.flags, c, data, True) is not None
                ok = memo[data]
            if not ok:
                out[r, t] = -np.inf
    return out


@pytest.mark.parametrize("V,rows", [(257, 1), (257, 9), (320, 2), (320, 9), (151936, 2)])
def test_apply_against_the_table_walker_bit_for_bit(jv, V, rows):
    g, walked = jv
    con, tokens = _device_grammar(g, V)
    order = ["in_array", "done", "one", "d63", "d64", "start", "closed", "obj", "d64s", "mid_char", "after_key", "three"]
    if rows <= 2:
        order = ["in_array", "one"] if V == 320 else ["d63", "done"] if V > 1000 else ["closed"]
    names = order[:rows]
    configs = [walked["three" if n == "done" else n] for n in names]
    done = [int(n == "done") for n in names]
    ld = V + 7
    rng = np.random.default_rng(V + rows)
    logits = rng.standard_normal((rows, ld)).astype(np.float32)
    logits[:, V:] = NAN                                           # behind every row, and so in front of the next
    for r in range(rows):
        if done[r]:
            logits[r] = NAN                                       # a done row is not touched at all
    logits[0, 5] = np.float32(-0.0)
    stops = [0, V - 1]                                            # the first and the last token; both have bytes
    want = _reference(g, tokens, logits, configs, done, stops)
    got = con.apply(logits, configs, done, stops)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (con.apply(logits, configs, done, stops).view(np.uint32) == got.view(np.uint32)).all()   # the same call, the same bits
    masked = np.isneginf(got[:, :V]) & ~np.isneginf(logits[:, :V])
    for r, n in enumerate(names):
        if n == "done":
            assert np.isnan(got[r]).all()
            continue
        assert masked[r].any() and not masked[r].all(), n
        assert masked[r, 0] == masked[r, V - 1] == (not GC.accepted(g.flags, configs[r])), n     # the stop rule, whatever the bytes
        assert masked[r, 1 + FIXED.index(b"")], n                 # no bytes: never allowed
    by = {n: r for r, n in enumerate(names)}
    if "in_array" in by:                                          # 16 own pushes live, 17 die
        assert not masked[by["in_array"], 1 + FIXED.index(b"[" * 8)] and masked[by["in_array"], 1 + FIXED.index(b"[" * 8 + b"1")]
    if "d63" in by:                                               # one level left: a scalar fits, a container does not
        assert not masked[by["d63"], 1 + FIXED.index(b"1")] and masked[by["d63"], 1 + FIXED.index(b"[")]
        assert not masked[by["d63"], 1 + FIXED.index(b"]]]")]     # three pops below the token's own (empty) window
    if "d64" in by:
        assert masked[by["d64"], 1 + FIXED.index(b",[")] and not masked[by["d64"], 1 + FIXED.index(b",")]
        assert not masked[by["d64"], 1 + FIXED.index(b"]],")]
    if "obj" in by:
        assert not masked[by["obj"], 1 + FIXED.index(b"{\"a\":[")] and not masked[by["obj"], 1 + FIXED.index(b"[]")]
    if "mid_char" in by:                                          # in the middle of é: only its second byte goes on
        assert not masked[by["mid_char"], 1 + FIXED.index(b"\xa9")] and masked[by["mid_char"], 1 + FIXED.index(b"\xc3\xa9")]
    if "three" in by:
        assert not masked[by["three"], 1 + FIXED.index(b"\"}]")] and not masked[by["three"], 1 + FIXED.index(b"\xc3\xa9")]


def test_apply_refusals_come_before_any_gpu_work(jv):
    import kjarni_amd
    g, walked = jv
    con, tokens = _device_grammar(g, 257)
    logits = np.zeros((1, 257), np.float32)
    for kwargs, word in ((dict(configs=[(g.states, ())]), "no state"), (dict(configs=[(0, (g.states,))]), "no state"),
                         (dict(configs=[(0, tuple([1] * 65))]), "depths"), (dict(configs=[GC.START], stop_ids=list(range(17))), "16")):
        with pytest.raises(kjarni_amd.KjarniException) as e:
            con.apply(logits, **kwargs)
        assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and word in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException):
        con.apply(np.zeros((1, 200), np.float32), [GC.START])     # ld below the vocabulary


# ---- advance alone ----------------------------------------------------------------------------------------------------------------------

def test_advance_every_ending_the_depth_limit_and_the_stack_above(jv):
    g, walked = jv
    con, tokens = _device_grammar(g, 320)
    tok = lambda data: 1 + FIXED.index(data)  # noqa: E731
    STOP = 319                                                    # "]": a stop id with bytes
    above = np.full(64, 0xEEEE, np.uint16)                        # what lies above the depth must stay
    cases = [  # (name, config, pick, done before) -> expectations computed from the walker below
        ("stop_accepted", walked["one"], STOP, 0), ("stop_not_accepted", walked["in_array"], STOP, 0), ("closes", walked["in_array"], tok(b"]"), 0),
        ("moves", walked["in_array"], tok(b"{\"a\":["), 0), ("pops_three", walked["three"], tok(b"\"}]"), 0), ("masked", walked["start"], tok(b"}"), 0),
        ("no_bytes", walked["start"], tok(b""), 0), ("out_of_range", walked["start"], 100000, 0), ("negative", walked["start"], -1, 0),
        ("done_before", walked["three"], tok(b"}"), 1), ("push_at_63", walked["d63"], tok(b"1"), 0), ("push_at_64", walked["d64"], tok(b",["), 0),
        ("pop_then_push_at_64", walked["d64"], tok(b","), 0), ("seventeen", walked["in_array"], tok(b"[" * 8 + b"1"), 0),
        ("sixteen", walked["in_array"], tok(b"[" * 8), 0), ("pops_to_the_end", GC.walk(g.action, g.flags, GC.START, b"[[[1"), tok(b"]]]"), 0),
    ]
    configs = [(c[0], c[1], above) for _, c, _, _ in cases]
    res = con.advance([p for _, _, p, _ in cases], configs, [d for _, _, _, d in cases], [STOP])
    for r, (name, c, pick, done) in enumerate(cases):
        before = above.copy()
        before[:len(c[1])] = c[1]
        if done:
            want, violated, end = c, 0, 1
        elif pick == STOP:
            ok = GC.accepted(g.flags, c)
            want, violated, end = c, int(not ok), 1
        else:
            nxt = GC.walk(g.action, g.flags, c, tokens[pick], True) if 0 <= pick < 320 and tokens[pick] else None
            want, violated = (c, 1) if nxt is None else (nxt, 0)
            end = int(nxt is None or GC.closed(g.flags, nxt))
        assert (int(res["states"][r]), int(res["depths"][r])) == (want[0], len(want[1])), name
        assert tuple(res["stacks"][r, :len(want[1])]) == want[1], name
        assert int(res["violated"][r]) == violated and int(res["done"][r]) == end, name
        low = min(len(c[1]), len(want[1]))
        if violated or done:
            assert (res["stacks"][r] == before).all(), name       # a refused pick moves nothing
        else:
            keep = np.ones(64, bool)
            keep[:len(want[1])] = False                           # below the new depth: the new stack (checked above)
            assert (res["stacks"][r][keep] == before[keep]).all(), name
            assert low <= len(c[1])
    by = {name: r for r, (name, _, _, _) in enumerate(cases)}
    assert res["violated"][by["stop_not_accepted"]] == 1 and res["violated"][by["stop_accepted"]] == 0
    assert res["done"][by["closes"]] == 1 and res["done"][by["moves"]] == 0
    assert res["depths"][by["push_at_63"]] == 64 and res["violated"][by["push_at_64"]] == 1 and res["depths"][by["pop_then_push_at_64"]] == 63
    assert res["violated"][by["seventeen"]] == 1 and res["depths"][by["sixteen"]] == 17
    assert res["depths"][by["pops_three"]] <= len(walked["three"][1]) - 3 and res["violated"][by["pops_three"]] == 0
    assert res["done"][by["pops_to_the_end"]] == 1 and res["violated"][by["pops_to_the_end"]] == 0
    assert res["done"][by["done_before"]] == 1 and res["violated"][by["done_before"]] == 0


def test_advance_logs_state_and_depth_behind_the_recorded_pick(jv):
    import kjarni_amd
    g, walked = jv
    con, tokens = _device_grammar(g, 320)
    c = walked["in_array"]
    nxt = GC.walk(g.action, g.flags, c, b"{\"a\":[", True)
    for count, where in ((3, 2), (1, 0), (4, 3), (5, None), (0, None)):
        res = con.advance([1 + FIXED.index(b"{\"a\":[")], [c], log_count=count, log_cap=4)
        want_s, want_d = np.full(4, 0xFFFFFFFF, np.uint32), np.full(4, -1, np.int32)
        if where is not None:
            want_s[where], want_d[where] = nxt[0], len(nxt[1])
        assert (res["state_log"] == want_s).all() and (res["depth_log"] == want_d).all(), count
    res = con.advance([1 + FIXED.index(b"}")], [c], log_count=1, log_cap=2)       # a masked pick logs the row as it stands
    assert res["violated"][0] == 1 and res["state_log"][0] == c[0] and res["depth_log"][0] == 1
    with pytest.raises(kjarni_amd.KjarniException):
        con.advance([1, 1], [c, c], log_count=1, log_cap=2)        # the log is for one row


# ---- the loops against the float64 oracle -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def llama(tmp_path_factory):
    import kjarni_amd
    d = str(tmp_path_factory.mktemp("grammar") / "llama")
    cfg, t = synth.llm_model(d, synth.LLAMA_TEST, seed=4)
    tokens = GC.model_tokens(cfg["vocab_size"])
    return kjarni_amd.HipDecoder(d, max_context=CAP), SC.Llama64(t, cfg), cfg, tokens, [2, 3]


@pytest.fixture(scope="module")
def gpt2(tmp_path_factory):
    import kjarni_amd
    d = str(tmp_path_factory.mktemp("grammar") / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=CAP)), seed=4)
    tokens = GC.model_tokens(cfg["vocab_size"], specials=(G.ENDOFTEXT,))
    return kjarni_amd.HipDecoder(d, 0), SC.Gpt264(t, cfg), cfg, tokens, [G.ENDOFTEXT]


_GRAMMARS = {}


def _grammar(rules, tokens, stops):
    key = (json.dumps(rules), id(tokens))
    if key not in _GRAMMARS:
        _GRAMMARS[key] = _K().GrammarConstraint(rules, tokens)
    con = _GRAMMARS[key]
    return con, GC.HostGrammar(con.grammar, tokens, stops)


def _prompt(seed, vocab, n=6):
    return np.random.default_rng(seed).integers(4, min(vocab, 700), n).tolist()


def _run(dec, con, loop, prompt, max_new, uniforms=None, stop_ids=None, on_token=None):
    dec.set_device_sampling(not loop.endswith("-host"))
    try:
        if loop.startswith("sampled"):
            return dec.generate_grammar(con, prompt, max_new, sample=True, uniforms=uniforms if max_new else None, stop_ids=stop_ids,
                                        on_token=on_token, **SAMPLED)
        return dec.generate_grammar(con, prompt, max_new, sample=False, repetition_penalty=1.0 if loop == "greedy" else PENALTY,
                                    stop_ids=stop_ids, on_token=on_token)
    finally:
        dec.set_device_sampling(True)


def _oracle(ref, hg, loop, prompt, max_new, uniforms=None, seed=0):
    if loop.startswith("sampled"):
        return CC.oracle_run(ref, prompt, max_new, hg, params=SAMPLED, uniforms=uniforms, seed=seed, context=CAP)
    return CC.oracle_run(ref, prompt, max_new, hg, penalty=1.0 if loop == "greedy" else PENALTY, context=CAP)


def _clear_case(ref, hg, loop, max_new, vocab, seeds=range(1, 40)):
    """The first seeded prompt whose oracle run clears the float bar at every decision (near-ties are no fair demand of f32)."""
    for seed in seeds:
        prompt = _prompt(seed, vocab)
        ids, info = _oracle(ref, hg, loop, prompt, max_new, seed=seed)
        if info["clear"] and ids:
            return prompt, ids, info
    raise AssertionError("precondition: no seeded prompt clears the float bar")


def _check_result(res, hg, ids, info=None):
    c = hg.config_after(ids)
    assert c is not None and res["violated"] == 0
    assert (res["final_state"], res["final_depth"]) == (c[0], len(c[1])) == (res["device_state"], res["device_depth"])
    assert res["accepted"] == int(GC.accepted(hg.flags, c))
    if info is not None:
        assert info["final_state"] == c and res["complete"] == int(info["complete"]) and res["accepted"] == int(info["accepted"])
    return c


@pytest.mark.parametrize("family", ["llama", "gpt2"])
@pytest.mark.parametrize("which", ["json", "lists"])
def test_the_five_loops_agree_with_the_float64_oracle(request, family, which):
    dec, ref, cfg, tokens, stops = request.getfixturevalue(family)
    rules = _K().json_value() if which == "json" else GC.rules_of(GC.LISTS)
    con, hg = _grammar(rules, tokens, stops)
    n_new = 12
    got = {}
    for loop in LOOPS:
        base = "sampled" if loop.startswith("sampled") else loop.replace("-host", "")
        if base not in got:
            got[base] = _clear_case(ref, hg, base, n_new, cfg["vocab_size"])
        prompt, want, info = got[base]
        assert info["clear"]
        ids, res = _run(dec, con, loop, prompt, n_new, uniforms=np.asarray(info["uniforms"] + [0.5] * n_new, np.float32)[:n_new])
        assert ids == want, (loop, which)
        _check_result(res, hg, ids, info)
        assert dec.resident() == (prompt + ids)[:dec.cache_len()], loop


@pytest.mark.parametrize("loop", LOOPS)
def test_a_grammar_with_no_call_equals_the_pattern_route(llama, loop):
    dec, _, cfg, tokens, stops = llama
    pattern = r"[a-e]+(?:, [a-e]+)*\."
    con, hg = _grammar([("s", pattern)], tokens, stops)
    regex = _K().Constraint(pattern, tokens)
    for seed in (1, 2):
        prompt = _prompt(seed, cfg["vocab_size"])
        u = np.random.default_rng(seed).random(14).astype(np.float32)
        ids, res = _run(dec, con, loop, prompt, 14, uniforms=u)
        length, resident = dec.cache_len(), dec.resident()
        dec.set_device_sampling(not loop.endswith("-host"))
        if loop.startswith("sampled"):
            want, wres = dec.generate_constrained(regex, prompt, 14, sample=True, uniforms=u, **SAMPLED)
        else:
            want, wres = dec.generate_constrained(regex, prompt, 14, sample=False, repetition_penalty=1.0 if loop == "greedy" else PENALTY)
        dec.set_device_sampling(True)
        assert ids == want and (length, resident) == (dec.cache_len(), dec.resident())
        assert (res["complete"], res["accepted"], res["violated"]) == (wres["complete"], wres["accepted"], wres["violated"])
        assert res["final_depth"] == res["device_depth"] == 0
    regex.close()


@pytest.mark.parametrize("loop", LOOPS)
def test_a_grammar_that_allows_every_string_equals_the_plain_loops(llama, loop):
    dec, _, cfg, _, _ = llama
    toks = _GRAMMARS.setdefault("universal", CC.universal_tokens(cfg["vocab_size"], 2))
    con, hg = _grammar([("s", r"(?:.|\n)*")], toks, [2])
    for seed, n_new in ((1, 9), (2, 20)):
        prompt = _prompt(seed, cfg["vocab_size"])
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


@pytest.mark.parametrize("loop", LOOPS)
def test_json_value_outputs_parse_or_are_live_prefixes(llama, loop):
    dec, _, cfg, tokens, stops = llama
    K = _K()
    con, hg = _grammar(K.json_value(), tokens, stops)
    for seed in (1, 2, 3):
        prompt = _prompt(20 + seed, cfg["vocab_size"])
        u = np.random.default_rng(seed).random(30).astype(np.float32)
        ids, res = _run(dec, con, loop, prompt, 30, uniforms=u)
        text = hg.text(ids)
        _check_result(res, hg, ids)                                # a live prefix, host and device in the same configuration
        assert all(t not in stops for t in ids)
        if res["complete"]:
            assert res["accepted"]
            json.loads(text.decode("utf-8"))
        else:
            assert len(ids) == 30


def test_a_run_that_reaches_depth_64_goes_on_without_a_65th_level(llama):
    """A vocabulary of openers with a single closer: the model nests until the limit, where the mask leaves the closer alone."""
    dec, _, cfg, _, stops = llama
    V = cfg["vocab_size"]
    toks = [b"" if i < 4 else b"]" if i == 9 else b"[[" if i % 3 == 0 else b"[" for i in range(V)]
    con, hg = _grammar(GC.rules_of([("top", GC.Call("v")), ("v", GC.Seq(GC.Lit("["), GC.Rep(GC.Call("v"), 0, 1), GC.Lit("]")))]), toks, stops)
    ids, res = _run(dec, con, "greedy", _prompt(3, V), 100)
    depths = [len(hg.config_after(ids[:n])[1]) for n in range(len(ids) + 1)]
    assert max(depths) == 64 and res["violated"] == 0
    at = depths.index(64)
    assert ids[at] == 9 and at < len(ids)                          # at the limit only the closer is left, and the run took it
    _check_result(res, hg, ids)


@pytest.mark.parametrize("loop", LOOPS)
def test_endings(llama, loop):
    dec, ref, cfg, tokens, stops = llama
    V = cfg["vocab_size"]
    base = "sampled" if loop.startswith("sampled") else loop.replace("-host", "")
    # (a) a closed configuration in the middle of a burst: behind the full stop nothing can follow; no stop token
    con, hg = _grammar([("top", "(?&w)\\."), ("w", "yes|no|maybe")], tokens, stops)
    prompt, want, info = _clear_case(ref, hg, base, 12, V)
    ids, res = _run(dec, con, loop, prompt, 12, uniforms=np.asarray(info["uniforms"] + [0.5] * 12, np.float32)[:12])
    assert ids == want and 2 <= len(ids) <= 6
    c = _check_result(res, hg, ids, info)
    assert res["complete"] and res["accepted"] and GC.closed(hg.flags, c)
    if loop != "greedy":
        assert dec.cache_len() == len(prompt) + len(ids) - 1     # nothing follows the token that closed the grammar
    # (b) max_new_tokens inside a string: not accepted, not complete
    con, hg = _grammar([("s", "\"[a-e]{60}\"")], tokens, stops)
    prompt = _prompt(5, V)
    u = np.random.default_rng(5).random(6).astype(np.float32)
    ids, res = _run(dec, con, loop, prompt, 6, uniforms=u)
    assert len(ids) == 6 and (res["accepted"], res["complete"], res["violated"]) == (0, 0, 0)
    _check_result(res, hg, ids)
    ids0, res0 = _run(dec, con, loop, prompt, 0)
    assert ids0 == [] and (res0["final_state"], res0["final_depth"], res0["accepted"]) == (0, 0, 0) and dec.cache_len() == len(prompt)
    # (c) the callback stops the run at token 2
    seen = []
    ids2, res2 = _run(dec, con, loop, prompt, 6, uniforms=u, on_token=lambda t: seen.append(t) or len(seen) < 2)
    assert ids2 == seen == ids[:2] and res2["complete"] == 0
    _check_result(res2, hg, ids2)
    # (d) a stop id in an accepted configuration: a number may always go on, so only the stop id ends it
    con, hg = _grammar([("s", "(?&n)"), ("n", "-?[0-9]+")], tokens, stops)
    ids3, res3 = _run(dec, con, loop, prompt, 30, uniforms=np.random.default_rng(7).random(30).astype(np.float32))
    c = _check_result(res3, hg, ids3)
    assert res3["complete"] == int(len(ids3) < 30) and (not res3["complete"] or res3["accepted"])


# ---- refusals and surface ----------------------------------------------------------------------------------------------------------------

def test_refusals_before_any_gpu_work(llama):
    import kjarni_amd
    dec, _, cfg, tokens, stops = llama
    V = cfg["vocab_size"]
    K = _K()
    dec.generate(_prompt(1, V), 3)
    before = dec.resident()
    # no token holds "}": behind {x the rule can neither go on nor end
    toks = [b"" if i < 4 else b"{" if i % 2 else b"x" for i in range(V)]
    stuck = K.GrammarConstraint([("s", r"\{(?:x|(?&s))\}")], toks)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_grammar(stuck, _prompt(1, V), 4)
    assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and "state" in str(e.value) and "'s'" in str(e.value)
    toks[9] = b"}"
    fine = K.GrammarConstraint([("s", r"\{(?:x|(?&s))\}")], toks)
    ids, res = dec.generate_grammar(fine, _prompt(1, V), 8)
    assert res["violated"] == 0
    # the JSON grammars on a vocabulary of whole characters: the states inside a character are not reachable, nothing is refused
    chars = [b"" if i < 4 else c.encode() for i, c in enumerate((list("{}[]\",:0123456789.-+eEtrufalsn\\ abé€😀") * 20)[:V])]
    for rules in (K.json_value(), K.json_value(True)):
        ids, res = dec.generate_grammar(K.GrammarConstraint(rules, chars), _prompt(2, V), 6)
        assert res["violated"] == 0 and len(ids) <= 6
    # another vocabulary, too many stop ids
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_grammar(K.GrammarConstraint(K.json_value(), tokens[:100]), _prompt(1, V), 3)
    assert "100" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_grammar(fine, _prompt(1, V), 3, stop_ids=list(range(100, 117)))
    assert "16" in str(e.value)
    dec.generate(_prompt(1, V), 0)
    assert before[:6] == dec.resident()[:6]                       # (the refused calls ran nothing: the model still answers)


def test_generator_and_chat_end_to_end(tmp_path):
    import kjarni_amd
    from kjarni_amd import Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    K = _K()
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen = Generator("gpt2", model_path=d)
    greedy = GenerationConfig(do_sample=False, max_new_tokens=24)
    prompt = "The quick brown fox"
    plain = gen.generate(prompt, greedy)
    schema = {"type": "object", "properties": {"answer": {"enum": ["yes", "no"]}, "path": {"type": "array", "items": {"$ref": "#"}, "maxItems": 2}},
              "required": ["answer"]}
    full = K.Grammar(K.json_schema(schema))
    gen.set_grammar(K.json_schema(schema))
    for config in (greedy, GenerationConfig(temperature=1.3, max_new_tokens=24), GenerationConfig(do_sample=False, max_new_tokens=24,
                                                                                                 repetition_penalty=1.2)):
        gen.seed(7)
        text = gen.generate(prompt, config)
        res = gen.grammar_result()
        assert res["violated"] == 0 and full.walk(full.start, text.encode()) is not None, text
        if res["complete"]:
            value = json.loads(text)
            assert value["answer"] in ("yes", "no") and full.matches(text.encode())
    gen.set_constraint(K.choices(["yes", "no", " maybe"]))           # a pattern clears the grammar ...
    assert gen.generate(prompt, greedy) in ("yes", "no", " maybe") and gen.constraint_result()["complete"] == 1
    gen.set_grammar([("s", "(?&w)!"), ("w", "yes|no")])             # ... and a grammar the pattern
    assert gen.generate(prompt, greedy) in ("yes!", "no!") and gen.grammar_result()["complete"] == 1
    with pytest.raises(kjarni_amd.KjarniException):
        gen.set_grammar([("s", "(?&s)a|a")])
    assert gen.generate(prompt, greedy) in ("yes!", "no!")          # a refused grammar leaves the old one in place
    gen.set_grammar(None)
    assert gen.generate(prompt, greedy) == plain                    # None restores the plain behaviour exactly
    gen.close()

    ld = str(tmp_path / "llama")
    synth.llm_model(ld, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(ld, "tokenizer.json"))
    chat = Chat("llama3.2-1b-instruct", model_path=ld)
    cfg = GenerationConfig(do_sample=False, max_new_tokens=16)
    plain = chat.send("Is water wet?", cfg)
    chat.set_grammar([("s", "\\[(?&w)(?:,(?&w))?\\]"), ("w", "Yes|No")])
    reply = chat.send("Is water wet?", cfg)
    assert reply in ("[Yes]", "[No]", "[Yes,Yes]", "[Yes,No]", "[No,Yes]", "[No,No]")
    assert chat.grammar_result()["complete"] == 1 and chat.grammar_result()["violated"] == 0
    chat.set_constraint(K.choices(["Yes.", "No."]))
    assert chat.send("Is water wet?", cfg) in ("Yes.", "No.")
    chat.set_constraint(None)
    assert chat.send("Is water wet?", cfg) == plain
